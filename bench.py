#!/usr/bin/env python
"""bench.py -- edited views/sec @512x512 (ControlNet denoise + splat render+bwd) on N MI355X GPUs.

One "step" = one chunk of `chunk_size` views pushed through the whole hot path:
  (a) eval render of each view (rgb + depth + alpha, one fused compositing sweep)            [rasterizer fwd]
  (b) 20-step CFG ControlNet+UNet cross-view denoise of the chunk against the 4 reference views' K/V.
      The reference trajectory (4 views) is computed INSIDE the timed region once per scene,
      i.e. each chunk pays its share of the reference work (V=40, c=3 -> 20/14 DDIM steps per chunk).
  (c) VAE decode of the chunk's edited latents
  (d) one training render of each view, forward + backward to the six Gaussian parameter tensors with the fused
      L1+SSIM loss against the edited image, the chunk's gradient sum all-reduced over ranks (RCCL) when N > 1.
Workload (BASELINE.json configs[1]): "bear"-like scene, V=40 views, 4 reference views, chunk_size=3, ~1M synthetic
Gaussians, SD1.5 + ControlNet-depth shapes with seeded random weights (no checkpoints / network), bf16.

Prints ONE JSON line on rank 0.  N > 1 (launched by torch.distributed.run, one rank per GPU): the views of ONE scene are
sharded over the ranks (view v -> rank v % N: 40 views = 5 per GPU at N = 8; `--views 80 --gaussians 2000000` is BASELINE
configs[2]); a step is one chunk on every rank.  Collectives on the measured path:
  1. the reference K / V^T bank of the NEXT scene: its owner rank (rotating, scene % N) runs the 4-view trajectory and
     broadcasts each DDIM step's K / V^T as one flat async RCCL message while everybody edits the current scene
     (`--ref-mode owner0` pins the owner, `--ref-mode replicate` is the A/B without the collective);
  2. one flat all-reduce of the chunk's N x 59 fp32 gradient sum, posted asynchronously from the buffer the backward
     kernel wrote into (two buffers alternate; it completes under the next chunk's denoise).

A plain run does what the headline needs and nothing else: setup, the untimed priming and `--warmup` steps, the `--steps` timed steps,
`--dump-outputs` if given, and the JSON line.  `--full` adds, after the timed steps and on rank 0: the roofline of the dominant denoise
kernel and of the rasterizer chain (instrumented extra steps; GC_BENCH_SHAPES=1 prints the per-shape GEMM table of the first), the f16 and
fp8 secondary measurements (N = 1, bf16 runs) and the CPU baseline (N = 1).  Without it those fields of the line are null.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

UNET_GFLOP_XVIEW = 1293.3      # per sample-forward, SURVEY.md Appendix B (analytic, 2*MAC)
CN_GFLOP_XVIEW = 430.0         # ControlNet with the weight-0 self term skipped
# CFG-shared prefix (sd.unet.AttnCtx.share, round 5): conv_in, the first resnet and the first transformer block up to its cross-view self-attention
# are computed for ONE of the two identical CFG halves.  GFLOP of that prefix per sample: UNet = 5 K/V sets x 4 L^2 C (107.4) + 2 convs 64^2
# 320 -> 320 (15.1) + GroupNorm/proj_in/Q|K|V (3.4) + conv_in (0.2); ControlNet = 4 sets (85.9) + the same rest.  `mfma_util_step` counts the
# FLOP EXECUTED: a CFG pair costs 2 x per_sample - prefix.
UNET_PREFIX_GFLOP, CN_PREFIX_GFLOP = 126.1, 104.6
PEAK_TFLOPS = {"bf16": 2500.0, "f16": 2500.0, "fp8": 2500.0}      # fp8 run: the dominant kernel (attention) still computes in bf16


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=14)   # one scene of V=40 views at chunk_size 3 = 14 chunks (+ 1 reference trajectory)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gaussians", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=None)     # default: 40 (edit, BASELINE configs[1]) / 256 cameras (raster, configs[4])
    ap.add_argument("--chunk-size", type=int, default=None)   # views per step: 3 (edit, BASELINE configs[1]) / 8 (raster-only: one batched launch set per 8 cameras)
    ap.add_argument("--no-view-batch", action="store_true")   # render the views of a step one camera at a time (the round-4 path) instead of gsplat_ops.render_views
    ap.add_argument("--denoise-steps", type=int, default=20)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16", "fp8"])     # fp8: e4m3 resnet convs + C = 640 / 1280 transformer linears on the block-scaled MFMA, bf16 elsewhere
    ap.add_argument("--fp8-min-hw", type=int, default=256)   # with --dtype fp8: smallest map (pixels) whose resnet convs run on e4m3 (256: 16 x 16 maps, k-sliced; 1024: round-3 behaviour)
    ap.add_argument("--fp8-linears", type=int, default=0)     # with --dtype fp8: bit mask of the C = 640 / 1280 transformer linears that also run on e4m3 (weights.add_fp8_linears).
                                                              # Default 0 since round 5: e4m3 convolutions + the bf16 transformer blocks WITH the LayerNorm fold and the graph
                                                              # merges beat e4m3 linears without them (9.83 vs 9.66 views/s same box, profiles/r05_fp8_hybrid_ab.txt); 7 = round 4
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--workload", default="edit", choices=["edit", "raster", "full"])   # full: SURVEY.md 8d's optional whole-pipeline number (N = 1)
    ap.add_argument("--train-iters", type=int, default=500)     # --workload full: Adam iterations after the edit (gc_trainer.py:186-201)
    ap.add_argument("--ref-mode", default="rotate", choices=["rotate", "owner0", "replicate", "allgather"])    # N > 1: who computes the reference bank
    # (allgather: the reference trajectory sharded by sample, K / V^T all-gathered per attention layer; N in {2, 4, 8})
    ap.add_argument("--inflight", type=int, default=2)         # launch sets in flight on independent HIP stream pairs (1: strictly one after the other)
    ap.add_argument("--cobatch", type=int, default=4)          # consecutive chunks of a scene that share ONE launch set (GaussCtrlPipelineConfig.chunks_per_launch): against
                                                              # the cached reference bank a view's result does not depend on what shares its network batch, so `cobatch` chunks of
                                                              # chunk_size views run as one batch of cobatch x chunk_size -- every GEMM sees that many times the rows (the 384-row level-3
                                                              # problems fill a round; same box: 10.30 / 10.47 / 10.88 / 10.88 views/s at 2 / 3 / 4 / 7, profiles/r06_cobatch_sweep.txt).  A step stays ONE chunk; 1 = rounds 1-5
    ap.add_argument("--no-secondary", action="store_true")     # skip the short f16 secondary measurement (default workload, N = 1)
    ap.add_argument("--mask", action="store_true")   # BASELINE configs[3]: edits composited through a (synthetic elliptical) mask, gc_pipeline.py:226-234
    ap.add_argument("--dump-outputs", default=None, metavar="DIR")   # after the timed steps: what the last one computed as DIR/<name>.npy (write_outputs)
    ap.add_argument("--full", action="store_true")   # also the rooflines, the f16 / fp8 secondaries and the CPU baseline (--no-secondary / --no-cpu-baseline
                                                     # drop one of them again); not the same thing as `--workload full`
    return ap.parse_args()


class GemmProfiler:
    """Brackets every gc_dn_gemm launch with HIP events on the launch stream (one instrumented step)."""

    def __init__(self, dt="BF16"):
        self.rec = []
        self.shapes = []            # (op, M, N, K, flags, start, end) of every linear / conv launch (GC_BENCH_SHAPES=1: per-shape table on stderr)
        self.dt = dt
        self.true_cin = {}          # e4m3 conv weight pointer -> un-padded input channels (the fp8 convs pad Cin to 128)
        self.att_kinds = []         # (kernel, frames, queries per frame, K/V sets, start, end) of every attention launch

    @staticmethod
    def _given(v):
        return v is not None and v is not False and not (isinstance(v, (int, float)) and v == 0)

    def wrap(self, ops):
        self._lin, self._conv, self._att = ops.linear, ops.conv3x3, ops.attention
        self._tail, self._head = ops.transformer_tail, ops.transformer_head
        self._lin8, self._conv8 = ops.linear_fp8, ops.conv3x3_fp8
        prof = self

        def lin8(x8, w8, *a, **k):          # e4m3 operands on v_mfma_scale_f32_16x16x128_f8f6f4 (k_gemm8q): priced against the 5 PF e4m3 peak
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._lin8(x8, w8, *a, **k)
            e.record()
            K = x8.shape[-1]
            prof.rec.append(("gemm8q<e4m3,linear> (block-scaled MFMA, dn_gemm_fp8.hip)", 2.0 * (x8.numel() // K) * w8.shape[0] * K, s, e))
            return out

        def conv8(x8, w8, *a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._conv8(x8, w8, *a, **k)
            e.record()
            o = out[0] if isinstance(out, tuple) else out
            # algorithmic FLOP on the TRUE input channels would need the unpadded Cin; every fp8 conv here has Cin % 128 == 0 except 320 / 960 / 1920
            # (padded to 384 / 1024 / 1920): count the padded K the kernel multiplies? No -- algorithmic = the bf16 path's 2 M N 9 Cin.
            cin = prof.true_cin.get(w8.data_ptr(), w8.shape[1] // 9)
            prof.rec.append(("gemm8q<e4m3,conv3x3> (block-scaled MFMA, dn_gemm_fp8.hip)", 2.0 * (o.numel() // o.shape[-1]) * w8.shape[0] * 9 * cin, s, e))
            return out

        def att(q, k, vt, heads, sets, fph, Lk=None, **kw):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._att(q, k, vt, heads, sets, fph, Lk=Lk, **kw)
            e.record()
            lk = k.shape[1] if Lk is None else Lk
            D = q.shape[2] // heads
            fast = D in (40, 80) and len(sets) * ((lk + 63) // 64) >= 4                      # mirrors launch_attn() in dn_attn.hip
            variant = getattr(ops, "KERNEL_VARIANT", {}).get("attn", 0)
            if fast and D == 40 and not (variant & 30) and lk % 64 == 0 and q.shape[1] % 256 == 0:
                name = f"k_attn5<{prof.dt},40> (8 waves, key-split)"
            elif fast and D == 40 and not (variant & 2):
                name = f"k_attn4<{prof.dt},40,3,{8 if variant & 4 else 4}>"
            else:
                name = f"k_attn3<{prof.dt},{D},{2 if D == 40 else 1},3>" if fast else f"k_attn<{prof.dt},{D},{1 if D == 160 else 2}>"
            prof.rec.append((name, 4.0 * q.shape[0] * q.shape[1] * lk * q.shape[2] * len(sets), s, e))
            prof.att_kinds.append((name, int(q.shape[0]), int(q.shape[1]), len(sets), s, e))
            return out

        def lin(x, w, *a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._lin(x, w, *a, **k)
            e.record()
            K = x.shape[-1]
            N = w.shape[-2]                                                                   # ([S, N, K] weight sets: the text-attention fold)
            ntw = 5 if ((N % 160 == 0 and N % 128 != 0 and not k.get("geglu", False)) or k.get("softmax_keys", 0)) else 4      # mirrors plan() in dn_gemm.hip
            prof.rec.append((f"gemm<{prof.dt},linear,BN={32 * ntw}>", 2.0 * (x.numel() // K) * N * K, s, e))
            prof.shapes.append(("linear", x.numel() // K, N, K, "+".join(f for f in ("geglu", "ln", "residual", "out_t", "softmax_keys", "chan_parts") if prof._given(k.get(f))), s, e))
            return out

        def conv(x, w, *a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._conv(x, w, *a, **k)
            e.record()
            N = w.shape[0]
            ntw = 5 if (N % 160 == 0 and N % 128 != 0) else 4
            mode = 2 if x.shape[-1] % 64 == 0 else 1
            o = out[0] if isinstance(out, tuple) else out              # (out, ChanParts) when the producer statistics were asked for
            prof.rec.append((f"gemm<{prof.dt},conv3x3{'' if mode == 2 else ' generic'},BN={32 * ntw}>", 2.0 * (o.numel() // o.shape[-1]) * N * w.shape[1], s, e))
            prof.shapes.append(("conv3x3", o.numel() // o.shape[-1], N, w.shape[1], f"hw={o.shape[1]}x{o.shape[2]}" if o.dim() == 4 else "", s, e))
            return out

        def tail(o, h, x, *a, **k):      # level-0 block after the attention, one launch: 2 * rows * 1.6896 M weights (incl. the 77-key text attention)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._tail(o, h, x, *a, **k)
            e.record()
            C_ = o.shape[-1]
            prof.rec.append((f"k_ttail<{prof.dt}> (row-resident block tail)", 2.0 * (o.numel() // C_) * (4 * C_ * C_ + 12 * C_ * C_ + 2 * 77 * C_), s, e))
            return out

        def head(x, *a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = prof._head(x, *a, **k)
            e.record()
            C_ = x.shape[-1]
            prof.rec.append((f"k_thead<{prof.dt}> (row-resident block head)", 2.0 * (x.numel() // C_) * 4 * C_ * C_, s, e))
            return out

        ops.linear, ops.conv3x3, ops.attention = lin, conv, att
        ops.transformer_tail, ops.transformer_head = tail, head
        ops.linear_fp8, ops.conv3x3_fp8 = lin8, conv8

    def unwrap(self, ops):
        ops.linear, ops.conv3x3, ops.attention = self._lin, self._conv, self._att
        ops.transformer_tail, ops.transformer_head = self._tail, self._head
        ops.linear_fp8, ops.conv3x3_fp8 = self._lin8, self._conv8

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for kind, fl, s, e in self.rec:
            d = out.setdefault(kind, {"launches": 0, "flop": 0.0, "ms": 0.0})
            d["launches"] += 1; d["flop"] += fl; d["ms"] += s.elapsed_time(e)
        return out


VAE_DECODE_GFLOP = 1240.0      # AutoencoderKL decoder, 64x64 latents -> 512x512 (~1.2 TFLOP / frame)


class Bench:
    """State of one benchmark stream on this rank: scene, cameras, networks, reference banks, gradient buffers."""

    def __init__(self, args, dtype_name, rank, world, dev, dist, bank_group):
        from gaussctrl_amd import gsplat_ops as gops, synthetic as syn
        from gaussctrl_amd.camera import camera_to_gsplat
        from gaussctrl_amd.dist import FlatGrads, shard_views
        from gaussctrl_amd.sd import arch, ops as sdops
        from gaussctrl_amd.sd.pipeline import DenoisePipeline
        from gaussctrl_amd.sd.vae import prepare_vae_weights
        from gaussctrl_amd.sd.weights import prepare
        from gaussctrl_amd.train_ops import l1_ssim_loss, l1_ssim_loss_views
        self.args, self.rank, self.world, self.dev, self.dist, self.bank_group = args, rank, world, dev, dist, bank_group
        self.gops, self.sdops, self.l1_ssim_loss, self.l1_ssim_loss_views = gops, sdops, l1_ssim_loss, l1_ssim_loss_views
        self.view_batch = not args.no_view_batch          # the views of a step through ONE set of launches (gsplat_ops.render_views)
        self.dtype_name = dtype_name
        self.dt = dt = torch.float16 if dtype_name == "f16" else torch.bfloat16
        self.edit = args.workload == "edit"
        self.c, self.V, self.nsteps = args.chunk_size, args.views, args.denoise_steps
        self.H = self.W = H = W = 512
        K = syn.BEAR_INTRINSICS if self.edit else syn.ROUND_INTRINSICS      # config 5 uses fx=fy=540, cx=cy=256
        V, c = self.V, self.c
        # ------------------------------------------------------------ scene, cameras, networks (untimed setup)
        P = syn.make_gaussians(args.gaussians, seed=0)
        self.params = {k: torch.tensor(v, device=dev, requires_grad=True) for k, v in P.items()}
        self.ref_mode = args.ref_mode if (world > 1 and self.edit) else "local"
        if self.edit:
            # ONE scene of V views sharded over the ranks.  With a bank owner (rotate / owner0) the sharding is load balanced
            # (gaussctrl_amd.dist.shard_views_balanced): the rank that computes the NEXT scene's reference trajectory during this scene
            # edits ~4 views fewer, everybody else correspondingly more, and every rank's views are spread evenly over the scene's cps
            # lock-step chunks.  Replicated bank / N = 1: plain v % N sharding in chunks of chunk_size.
            from gaussctrl_amd.dist import shard_views_balanced, split_chunks
            cams = syn.make_cameras(V, seed=1)
            if self.ref_mode in ("rotate", "owner0"):
                most = max(len(shard_views_balanced(V, world, r, 0)) for r in range(world))
                self.cps = math.ceil(most / c)

                def chunks_of(scene, _cache={}):
                    o = self.owner_of(scene + 1)
                    if o not in _cache:
                        _cache[o] = split_chunks(shard_views_balanced(V, world, rank, o), self.cps, c)
                    return _cache[o]
            else:
                mine = shard_views(V, world, rank)
                self.cps = math.ceil(math.ceil(V / world) / c)               # chunks per scene on every rank (ranks stay in lock step)
                plain = [mine[j * c:(j + 1) * c] for j in range(self.cps)]   # the last chunk of a scene is short (40 = 13 x 3 + 1), gc_pipeline.py:190
                chunks_of = lambda scene: plain
            self.chunks_of = chunks_of
            self.mine = list(range(V))              # cameras of every view (the balanced shards move with the owner)
        else:
            # raster-only (configs[4]): every rank renders its own V random cameras of the same 4 M-Gaussian scene
            cams = syn.make_cameras(V * world, seed=1)[rank * V:(rank + 1) * V]
            self.mine = list(range(V))
            self.cps = math.ceil(V / c)
            self.chunks_of = lambda scene: [self.mine[j * c:(j + 1) * c] for j in range(self.cps)]
        self.ref_idx = [min(i, V - 1) for i in (4, 11, 29, 31)]                    # gc_pipeline.py:109-113 for V=40
        self.cams = {v: camera_to_gsplat(cams[v], K["fx"], K["fy"], K["cx"], K["cy"], W, H)
                     for v in sorted(set(self.mine) | (set(self.ref_idx) if self.edit else set()))}
        self.bg = torch.zeros(3, device=dev)
        self.pipe = None
        if self.edit:
            # LayerNorm fold (round 5 default): the LayerNorms of the C = 640 / 1280 transformer blocks live in their producer / consumer GEMM
            # epilogues (weights.prepare(fold_ln=2), dn_gemm_ln.hip).  GC_DN_FOLD_LN=0 restores the stand-alone kernels (A/B), 1 folds every
            # block (the C = 320 ones then leave the row-resident head / tail kernels).  The fp8 linears take e4m3 from the LayerNorm kernel: no fold.
            fold_ln = int(os.environ.get("GC_DN_FOLD_LN", "0" if (dtype_name == "fp8" and args.fp8_linears) else "2"))
            usd, csd = arch.random_state_dict(arch.unet_shapes(), 100, dev), arch.random_state_dict(arch.controlnet_shapes(), 200, dev)
            uw = prepare(usd, dt, dev, heads=8, fold_ln=fold_ln)
            cw = prepare(csd, dt, dev, heads=8, fold_ln=fold_ln)
            if dtype_name == "fp8":
                from gaussctrl_amd.sd.weights import add_fp8_convs, add_fp8_linears
                add_fp8_convs(uw, usd, dev); add_fp8_convs(cw, csd, dev)
                if args.fp8_linears and not fold_ln:      # C = 640 / 1280 transformer linears on e4m3 (bit 0 feed-forward, 1 attn2.to_q, 2 Q | K | V)
                    add_fp8_linears(uw, args.fp8_linears); add_fp8_linears(cw, args.fp8_linears)
            del usd, csd
            vw = prepare_vae_weights(arch.random_state_dict(arch.vae_decoder_shapes(), 300, dev), dt, dev)
            self.pipe = DenoisePipeline(uw, cw, vw, self.nsteps, 5.0)
            self.pipe.unet.fuse_stats = self.pipe.controlnet.fuse_stats = os.environ.get("GC_DN_FUSE_GN", "0") != "0"
            self.pipe.unet.gn_two_pass = self.pipe.controlnet.gn_two_pass = os.environ.get("GC_DN_GN2", "0") != "0"
        g = torch.Generator(device=dev).manual_seed(2)                             # the same scene inputs on every rank
        self.ctx_neg = torch.randn(1, 77, 768, device=dev, generator=g)
        self.ctx_pos = torch.randn(1, 77, 768, device=dev, generator=g)
        self.z0 = torch.randn(V, 4, 64, 64, device=dev, generator=g)              # stand-in for the DDIM-inverted latents
        self.stats = {"M": [], "dev": []}
        self.state = {"bank": None, "next": None, "cap": None, "views_done": 0, "renders_done": 0}
        self.syncfree = os.environ.get("GC_BENCH_SYNCFREE", "1") != "0"
        self.sorted_boxes = os.environ.get("GC_RASTER_SORTED_BOXES", "1") != "0"      # 0: the round-5 depth-order chain (pairs + two gathers), A/B
        self.raster_target = torch.rand(H, W, 3, device=dev, generator=g)     # raster-only workload: a fixed synthetic target image
        self.edit_mask = torch.tensor(syn.elliptical_mask(H, W, soft=True), device=dev, dtype=torch.float32) if args.mask else None
        # the chunk's summed leaf gradients: six views of ONE flat buffer that the backward kernel writes into and RCCL reduces in
        # place; two buffers alternate so the all-reduce of chunk k completes under the denoise of chunk k + 1
        self.grads = [FlatGrads(self.params) for _ in range(max(2 if world > 1 else 1, max(1, args.inflight) if args.workload == "edit" else 1))]
        self.bank_layers = None
        # consecutive chunks are independent given the reference bank: each runs on its own stream (pair), `inflight` of them at a time,
        # so the part-filled grids and the fill / drain phases of one chunk's kernels are covered by the other's; the next scene's
        # reference trajectory has a stream of its own
        self.inflight = max(1, args.inflight) if self.edit else 1
        self.cobatch = max(1, min(args.cobatch, max(1, 21 // max(1, args.chunk_size or 3)))) if self.edit else 1          # (a launch set is validated up to 21 views)
        self.sets_done = 0
        self.streams = [torch.cuda.Stream(device=dev) for _ in range(self.inflight)] if self.inflight > 1 else [None]
        self.ref_stream = torch.cuda.Stream(device=dev) if self.inflight > 1 else None
        self.bank_ready = None          # event on ref_stream: the bank the chunks are about to use is complete
        self.half_events = []           # (start, end of denoise half, end of step) HIP events of the timed steps
        self.record_halves = False
        self.rank0_only = False
        self.keep = None                # a dict (--dump-outputs): every launch set leaves what it computed here, the last one wins

    # ------------------------------------------------------------------------------------------------ pieces of a step
    def new_aux(self):
        aux = self.gops.RenderAux()
        aux.sorted_boxes = self.sorted_boxes
        if self.syncfree and self.state["cap"]:
            aux.m_cap = self.state["cap"]          # device-side intersection count + capacity: no host round trip in the frame
        return aux

    def note_m(self, aux, sized_on_host=False):
        if isinstance(aux.M, tuple) and sized_on_host:      # a view batch that read its counts back to size the lists (first frames)
            cnts = [int(v) for v in aux.M[0].cpu().reshape(-1)]
            self.stats["M"] += cnts
            self.state["cap"] = max(self.state["cap"] or 0, int(max(cnts) * 1.3) + 1024)
        elif isinstance(aux.M, tuple):
            self.stats["dev"].append(aux.M)        # (count, overflow) device tensors: read after the timed region
        else:
            self.stats["M"].append(aux.M)
            self.state["cap"] = max(self.state["cap"] or 0, int(aux.M * 1.3) + 1024)

    def render_eval(self, i):
        p, aux = self.params, self.new_aux()
        with torch.no_grad():
            rgb, alpha, depth = self.gops.render_view(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"],
                                                      self.cams[i], self.bg, True, 3, aux)
        self.note_m(aux)
        return rgb, depth, aux

    def render_eval_views(self, views):
        """the eval renders of a step's views as ONE batched launch set -> [(rgb, depth, aux)] per view"""
        if not self.view_batch or len(views) < 2:
            return [self.render_eval(i) for i in views]
        p, aux = self.params, self.new_aux()
        with torch.no_grad():
            rgb, alpha, depth = self.gops.render_views(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"],
                                                       [self.cams[i] for i in views], self.bg, True, 3, aux)
        self.note_m(aux, sized_on_host=aux.m_cap is None)
        return [(rgb[k], depth[k], aux) for k in range(len(views))]

    def disparity_of(self, depth):            # gc_pipeline.py:258-266 as one HIP kernel pair -> [H,W,8] control image (3 channels used)
        return self.sdops.depth_to_disparity(depth, self.dt)

    def ref_inputs(self):
        rd = torch.stack([self.disparity_of(self.render_eval(i)[1]) for i in self.ref_idx])
        return self.z0[self.ref_idx], rd, self.ctx_neg, self.ctx_pos

    def owner_of(self, scene):
        return scene % self.world if self.ref_mode == "rotate" else 0

    def begin_bank(self, scene):
        """the reference bank of `scene` as a trajectory that advance_bank() moves: local (N = 1 / replicate) or a RefBankStream"""
        if self.ref_mode in ("local", "replicate"):
            return self.pipe.begin_ref_bank(*self.ref_inputs())
        if self.ref_mode == "allgather":
            from gaussctrl_amd.dist import RefShard
            return self.pipe.begin_ref_bank_sharded(*self.ref_inputs(), RefShard(self.world, self.rank, group=self.bank_group))
        from gaussctrl_amd.dist import RefBankStream
        st = RefBankStream(self.pipe, self.owner_of(scene), self.world, self.rank, self.dev, self.nsteps, group=self.bank_group,
                           layers=self.bank_layers)
        return st.begin(*self.ref_inputs()) if st.owner else st

    def advance_bank(self, tr, n):
        """n more DDIM steps (None: all); returns the finished RefBank or None"""
        if isinstance(tr, dict):
            return self.pipe.advance_ref_bank(tr, n)
        tr.drain(0)                       # what the previous chunk posted has had a whole chunk to arrive: unpack it now
        done = tr.advance(n)
        self.bank_layers = tr.layers
        return tr.finish() if done else None

    def groups(self, g0, n):
        """the n steps (chunks) g0 .. g0 + n - 1 as launch sets: up to `cobatch` consecutive chunks of ONE scene share a set"""
        out, s, end = [], g0, g0 + n
        while s < end:
            k = 1
            # (sets are aligned to multiples of `cobatch` inside a scene, wherever the timed region starts: the short last chunk of a scene
            # always shares its set with the chunk before it)
            while k < self.cobatch and s + k < end and (s + k) // self.cps == s // self.cps and ((s + k) % self.cps) % self.cobatch != 0:
                k += 1
            out.append(list(range(s, s + k)))
            s += k
        return out

    def step(self, s):
        """one launch set: chunk s, or the list of co-batched chunks"""
        ss = [s] if isinstance(s, int) else list(s)
        st_ = self.streams[self.sets_done % len(self.streams)]
        self.sets_done += 1
        if st_ is None:
            return self._step(ss)
        with torch.cuda.stream(st_):
            return self._step(ss)

    def _step(self, ss):
        """Chunks ss (consecutive, one scene) of an endless stream of scenes (cps chunks per scene on every rank) as ONE launch set.  A scene's
        reference trajectory (4 views x 20 DDIM steps, shared by its chunks) is computed while the PREVIOUS scene is edited, 20 / cps DDIM
        steps per chunk, so every step carries exactly its share of the reference work whatever K is."""
        st, c, cps, nsteps, p = self.state, self.c, self.cps, self.nsteps, self.params
        s = ss[0]
        scene, j = divmod(s, cps)
        j1 = j + len(ss) - 1                       # last chunk of the set (same scene)
        assert (ss[-1]) // cps == scene
        views = [v for jj in range(j, j1 + 1) for v in self.chunks_of(scene)[jj]]
        st["views_done"] += len(views)
        ev = None
        if self.record_halves:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        if self.edit:
            cur = torch.cuda.current_stream()
            refs = self.ref_stream if self.ref_stream is not None else cur
            with torch.cuda.stream(refs):
                if st["bank"] is None:                # the very first scene (setup): its whole reference trajectory at once
                    st["bank"] = self.advance_bank(self.begin_bank(scene), None)
                    self.bank_ready = torch.cuda.Event(); self.bank_ready.record()
                if st["next"] is None:                # the following scene's references start with this scene
                    st["next"] = self.begin_bank(scene + 1)
                quota = (nsteps * (j1 + 1)) // cps - (nsteps * j) // cps          # the reference share of every chunk of the set
                done = self.advance_bank(st["next"], quota)          # owner: compute + post sends; others: post receives (they arrive under (b))
            if self.bank_ready is not None:
                cur.wait_event(self.bank_ready)       # (no-op on the stream that recorded it)
            evals = self.render_eval_views(views)                                                           # (a)
            if views:
                disp = torch.stack([self.disparity_of(e[1]) for e in evals])
                lat = self.pipe.edit_chunk_cached(self.z0[views], disp, self.ctx_neg, self.ctx_pos, st["bank"])   # (b)
                edited = self.pipe.decode(lat)                                                              # (c)
            if j1 == cps - 1:
                assert done is not None
                st["prev_bank"] = st["bank"]          # chunks still in flight on other streams read it: keep it alive for one more scene
                st["bank"], st["next"] = done, None
                if self.ref_stream is not None:
                    self.bank_ready = torch.cuda.Event()
                    self.bank_ready.record(self.ref_stream)
        else:
            edited = [None] * len(views)
        if ev:
            ev[1].record()
        fg = self.grads[(self.sets_done - 1) % len(self.grads)]            # (same index -> same stream when sets are in flight on several streams)
        fg.wait()                                 # the all-reduce posted two chunks ago (N > 1) has finished before its buffer is rewritten
        if self.view_batch and len(views) >= 2:                                                             # (d), batched: one launch set
            aux = self.new_aux()
            aux.grad_into, aux.grad_accumulate = fg.views, False
            rgb, alpha, _ = self.gops.render_views(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"],
                                                   [self.cams[i] for i in views], torch.rand(len(views), 3, device=self.dev), False, 3, aux)
            if edited[0] is not None:
                target = edited.permute(0, 2, 3, 1).contiguous() if torch.is_tensor(edited) else torch.stack([e.permute(1, 2, 0) for e in edited]).contiguous()
                if self.args.mask:
                    target = torch.stack([self.sdops.mask_composite(target[jj], evals[jj][0].contiguous(), self.edit_mask) for jj in range(len(views))])
            else:
                target = self.raster_target.expand(len(views), -1, -1, -1)
            losses = self.l1_ssim_loss_views(rgb, target, 0.2)
            losses.sum().backward()                                         # the chunk's gradient SUM, formed inside the projection backward
            self.note_m(aux, sized_on_host=aux.m_cap is None)
            st["renders_done"] += len(views)
            views_iter = []
            train_rgb, train_loss = [rgb.detach()], [losses.detach()]
        else:
            views_iter = list(enumerate(views))
            train_rgb, train_loss = [], []
        for jj, i in views_iter:                                                                            # (d), one camera at a time
            aux = self.new_aux()
            aux.grad_into, aux.grad_accumulate = fg.views, jj > 0      # the batch's gradient sum is formed inside the backward kernel
            rgb, alpha, _ = self.gops.render_view(p["means"], p["scales"], p["quats"], p["opacities"], p["features_dc"], p["features_rest"],
                                                  self.cams[i], torch.rand(3, device=self.dev), False, 3, aux)
            target = edited[jj].permute(1, 2, 0).contiguous() if edited[jj] is not None else self.raster_target
            if self.args.mask and edited[jj] is not None:          # edited inside the mask, the un-edited render outside (one HIP kernel)
                target = self.sdops.mask_composite(target, evals[jj][0].contiguous(), self.edit_mask)
            loss = self.l1_ssim_loss(rgb, target, 0.2)             # the product path's loss (fused L1 + SSIM value and gradient kernels)
            loss.backward()
            self.note_m(aux)
            st["renders_done"] += 1
            if self.keep is not None:
                train_rgb.append(rgb.detach()[None]); train_loss.append(loss.detach().reshape(1))
        if not views:
            fg.flat.zero_()                       # a rank without a view in this chunk contributes zeros to the reduction
        if self.dist is not None and not self.rank0_only:      # (the instrumented roofline steps run on rank 0 alone: no collective)
            fg.reduce_async(self.world)
        if self.keep is not None:                 # references only: read after the timed region, before anything else runs a step
            self.keep.clear()
            self.keep.update(views=views, last_chunk=len(self.chunks_of(scene)[j1]), grads=fg, train_rgb=train_rgb, train_loss=train_loss)
            if self.edit and views:
                self.keep.update(latents=lat, edited=edited)
        if ev:
            ev[2].record()
            self.half_events.append(ev)

    def finish(self):
        for fg in self.grads:
            fg.wait()
        for st_ in self.streams:
            if st_ is not None:
                torch.cuda.current_stream().wait_stream(st_)
        if self.ref_stream is not None:
            torch.cuda.current_stream().wait_stream(self.ref_stream)

    def barrier(self):
        torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
        torch.cuda.synchronize()

    def run(self, warmup, steps):
        """two untimed priming chunks (caching allocator, kernel attribute calls, per-prompt / per-timestep caches reach their steady
        state), `warmup` untimed steps, then EXACTLY `steps` timed steps between barriers; returns (seconds = max over ranks,
        views edited by this rank in the timed region, training renders in it)"""
        g = 0
        prime = 2 * self.cobatch
        # the timed region starts on a launch-set boundary of its scene (sets are aligned to multiples of `cobatch` inside a scene): a few more
        # UNTIMED priming chunks when 2 cobatch + warmup does not end on one -- otherwise the first timed set is a torn one no pipeline run ever launches
        while self.cobatch > 1 and ((prime + warmup) % self.cps) % self.cobatch != 0:
            prime += 1
        for i, grp in enumerate(self.groups(0, prime) + self.groups(prime, warmup)):
            self.step(grp); g += len(grp)
            if i < 2:
                torch.cuda.synchronize()      # the priming sets also fill the per-prompt / per-timestep caches every stream reads later
        self.finish()
        self.barrier()
        v0, r0 = self.state["views_done"], self.state["renders_done"]
        self.record_halves = True
        t0 = time.perf_counter()
        for grp in self.groups(g, steps):          # EXACTLY `steps` chunks, `cobatch` of them per launch set
            self.step(grp); g += len(grp)
        self.finish()
        self.barrier()
        dt_s = time.perf_counter() - t0
        self.record_halves = False
        self.next_step = g
        if self.dist is not None:
            tt = torch.tensor([dt_s], device=self.dev, dtype=torch.float64)
            self.dist.all_reduce(tt, op=self.dist.ReduceOp.MAX)
            dt_s = float(tt.item())
        if self.stats["dev"]:                      # sync-free frames: counts / overflow flags are read only now
            cnts = torch.cat([a.reshape(-1) for a, _ in self.stats["dev"]]).cpu()
            ovfs = torch.cat([b.reshape(-1) for _, b in self.stats["dev"]]).cpu()
            assert int(ovfs.max()) == 0, "intersection capacity exceeded in a sync-free frame: raise the capacity margin"
            self.stats["M"] += [int(v) for v in cnts]
            self.stats["dev"] = []
        return dt_s, self.state["views_done"] - v0, self.state["renders_done"] - r0

    def halves(self):
        """GPU seconds of the timed steps spent in the denoise half ((a) eval renders + disparity, (b), (c), reference share) and in
        the raster training half ((d): render fwd + fused loss + bwd [+ posting the all-reduce]), from HIP events on the launch stream"""
        torch.cuda.synchronize()
        dn = sum(e[0].elapsed_time(e[1]) for e in self.half_events) * 1e-3
        rs = sum(e[1].elapsed_time(e[2]) for e in self.half_events) * 1e-3
        return dn, rs


def run_full_pipeline(args):
    """SURVEY.md 8d, the optional whole-pipeline number: ONE scene through the product classes exactly as the reference's trainer drives them
    (/root/reference/gaussctrl/gc_trainer.py:186-201): render_reverse (eval render + VAE encode + DDIM inversion of all V views), edit_images
    (reference trajectory + chunks of `chunk_size`, decode), then `--train-iters` iterations of train_iteration (one random edited view per
    iteration: render fwd + L1/SSIM + backward + fused Adam).  BASELINE configs[1] sizes; synthetic SD1.5-shaped weights; N = 1 only.
    value = wall seconds for the scene (lower is better); the three phases are reported beside it."""
    import time
    import torch
    from gaussctrl_amd import synthetic as syn
    from gaussctrl_amd.gc_config import build_optimizers
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline, GaussCtrlPipelineConfig, SimpleDataManager
    from gaussctrl_amd.ns_compat import Cameras
    dev = "cuda:0"
    V = args.views or 40
    args.chunk_size = args.chunk_size or 3
    K = syn.BEAR_INTRINSICS
    cams = Cameras(syn.make_cameras(V, seed=1), K["fx"], K["fy"], K["cx"], K["cy"], 512, 512)

    def scene():
        model = GaussCtrlModel(GaussCtrlModelConfig(background_color="black"), params=syn.make_gaussians(args.gaussians, seed=0), device=dev)
        cfg = GaussCtrlPipelineConfig(edit_prompt="a polar bear", reverse_prompt="a bear", chunk_size=args.chunk_size,
                                      num_inference_steps=args.denoise_steps, dtype="f16" if args.dtype == "f16" else "bf16",
                                      synthetic_weights=True, inflight_chunks=args.inflight)
        return GaussCtrlPipeline(cfg, dev, datamanager=SimpleDataManager(cams, seed=3), model=model), model

    def run(pipe, model, iters):
        import random
        random.seed(11)
        t = [time.perf_counter()]
        pipe.render_reverse(); torch.cuda.synchronize(); t.append(time.perf_counter())
        pipe.edit_images(); torch.cuda.synchronize(); t.append(time.perf_counter())
        opts = build_optimizers(model)
        for s in range(iters):
            pipe.train_iteration(opts, 30000 + s)
        torch.cuda.synchronize(); t.append(time.perf_counter())
        return [b - a for a, b in zip(t, t[1:])]

    pipe, model = scene()
    for _ in range(max(0, args.warmup)):                   # untimed: one short pass warms the allocator and every kernel's first launch
        run(pipe, model, 20)
    for td in pipe.datamanager.train_data:
        for k in ("z_0_image", "unedited_image", "depth_image", "image"):
            td.pop(k, None)
    del pipe, model
    torch.cuda.empty_cache()
    pipe, model = scene()
    torch.cuda.synchronize()
    inv, edit, train = run(pipe, model, args.train_iters)
    total = inv + edit + train
    print(json.dumps({
        "metric": "full GaussCtrl pipeline, seconds per scene (DDIM inversion + edit + Adam iterations)", "value": round(total, 3), "unit": "s",
        "n_gpus": 1, "steps": 1, "warmup": args.warmup, "ms_per_step": round(total * 1e3, 1), "higher_is_better": False, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": f"full pipeline: {V} views 512x512, {args.gaussians} Gaussians, chunk {args.chunk_size}, {args.denoise_steps} DDIM steps, "
                               f"{args.train_iters} Adam iterations (BASELINE configs[1] sizes), product classes GaussCtrlPipeline.render_reverse / edit_images / train_iteration",
                   "weights": "synthetic SD1.5-shaped (no checkpoints on the build machines)"},
        "phases_s": {"render_reverse (render + VAE encode + inversion)": round(inv, 3), "edit_images": round(edit, 3),
                     f"train_iteration x {args.train_iters}": round(train, 3)},
        "edited_views_per_s_edit_phase": round(V / edit, 3), "train_iterations_per_s": round(args.train_iters / train, 1)}), flush=True)


_BENCH_ENV_DEFAULTS = {"GC_DN_FOLD_LN": None, "GC_DN_FUSE_GN": "0", "GC_DN_GN2": "0", "GC_BENCH_SYNCFREE": "1", "GC_RASTER_SORTED_BOXES": "1", "GC_BENCH_ONE_GPU": "0",
                       "GC_BENCH_BACKEND": "nccl"}


def effective_options(sdops, args):
    """{switch: value} this run used -- every sd.ops.KernelOptions field plus the bench-level environment toggles; (None, None) returns
    the product defaults in the same shape, so `is_product_default` is a plain equality."""
    import dataclasses
    from gaussctrl_amd.sd import ops as _ops
    o = dataclasses.asdict(_ops.KernelOptions() if sdops is None else sdops.OPTIONS)
    o["ablate"] = sorted(o["ablate"])
    for k, d in _BENCH_ENV_DEFAULTS.items():
        v = d if sdops is None else os.environ.get(k, d)
        if k == "GC_DN_FOLD_LN":            # default depends on the run: fold level 2 except with e4m3 linears (they take e4m3 from the LayerNorm kernel)
            dflt = "2" if (args is None or not (args.dtype == "fp8" and args.fp8_linears)) else "0"
            v = dflt if (sdops is None or v is None) else v
        o[k] = v
    return o


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run with N ranks on this node."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL across processes needs it on these hosts
    env.setdefault("OMP_NUM_THREADS", "8")
    rc = subprocess.call(cmd, env=env)
    if rc:
        raise SystemExit(rc)


def dry_run(rank, world):
    """GC_BENCH_DRY=1 (tests/test_bench_launch.py, no GPU): the launch + rendez-vous path only -- init_process_group on GC_BENCH_BACKEND
    (gloo), one all-reduce, one JSON line from rank 0.  No measurement."""
    import datetime
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group(os.environ.get("GC_BENCH_BACKEND", "gloo"), rank=rank, world_size=world, timeout=datetime.timedelta(minutes=2))
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"dry_run": True, "world": world, "sum_of_rank_plus_1": float(t.item())}), flush=True)
    dist.destroy_process_group()


def last_step_outputs(B):
    """What the last timed step handed back, as host arrays: its chunk's edited latents and images (denoise + VAE decode), training renders
    and losses, and the summed gradients of the six Gaussian parameter tensors.  The gradients cover the whole launch set of that step: its
    chunks share one backward pass (--cobatch)."""
    k, out = B.keep, {}
    n = k["last_chunk"]
    if "latents" in k:
        out["latents"], out["edited"] = k["latents"][-n:], k["edited"][-n:]
    if k["train_rgb"]:
        out["train_rgb"], out["train_loss"] = torch.cat(k["train_rgb"])[-n:], torch.cat(k["train_loss"])[-n:]
    for name, g in k["grads"].views.items():
        out["grad_" + name] = g
    return {name: t.detach().float().cpu().numpy() for name, t in out.items()}


DUMP_BYTES = 64_000_000


def write_outputs(d, arrays, budget=DUMP_BYTES):
    """arrays -> d/<name>.npy in float32, at most `budget` bytes in all.  When the whole set does not fit, an array larger than its equal
    share of the budget is replaced by a fixed sample of its elements: flat indices from a seeded generator, ascending, the same positions
    in every run with the same arguments."""
    os.makedirs(d, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in arrays.items()}
    fits = sum(a.nbytes for a in arrays.values()) + 1024 * len(arrays) <= budget
    share = (budget // max(1, len(arrays)) - 1024) // 4          # elements per array (1 KB for the .npy header)
    for name, a in arrays.items():
        if not fits and a.size > share:
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, share, replace=False))]
        np.save(os.path.join(d, name + ".npy"), a)
    print(f"bench.py: {len(arrays)} outputs of the last timed step written to {d}", file=sys.stderr, flush=True)


def main():
    args = parse()
    # the training renders draw their backgrounds from the default generators: seeded, so that every run of the same arguments has the same inputs
    torch.manual_seed(0)
    if args.workload == "full":
        assert args.gpus == 1, "--workload full is a single-GPU measurement"
        if args.dump_outputs:
            raise SystemExit("bench.py: --dump-outputs covers the edit and raster workloads (the timed steps of Bench.run)")
        return run_full_pipeline(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # a bare `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU under torch.distributed.run, rendez-vous on
        # 127.0.0.1 and a free port) -- the form `python -m torch.distributed.run ... bench.py --gpus N` keeps working unchanged
        return self_launch(args)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks (use --nproc-per-node {args.gpus})")
    if os.environ.get("GC_BENCH_DRY", "0") == "1":
        return dry_run(rank, world)
    # GC_BENCH_ONE_GPU=1 + GC_BENCH_BACKEND=gloo: every rank on cuda:0 over gloo -- exercises the N > 1 code path on a 1-GPU box
    # (a functional check only; its number means nothing).  The driver's multi-GPU runs use neither.
    if os.environ.get("GC_BENCH_ONE_GPU", "0") == "1":
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    bank_group = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("GC_BENCH_BACKEND", "nccl")
        tmo = datetime.timedelta(minutes=10)       # a rank that never arrives aborts the job instead of hanging the node
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world, timeout=tmo)
        if args.workload == "edit" and args.ref_mode != "replicate":
            # the reference-bank broadcasts get their own communicator (own RCCL stream): a 0.5 GB message never queues in front of
            # the gradient all-reduce and the two kinds of collective need no common order
            bank_group = dist.new_group(list(range(world)), backend=backend, timeout=tmo)
    else:
        dist = None

    from gaussctrl_amd.sd import ops as sdops
    sdops.configure(sdops.options_from_env(), fp8_min_hw=args.fp8_min_hw)       # experiment switches (GC_FUSED_TAIL=0, GC_ATTN_V=4, GC_ABLATE=gn, ...): default = product
    if args.views is None:
        args.views = 40 if args.workload == "edit" else 256
    if args.chunk_size is None:
        args.chunk_size = 3 if args.workload == "edit" else 8
    c, V, nsteps = args.chunk_size, args.views, args.denoise_steps
    H = W = 512
    B = Bench(args, args.dtype, rank, world, dev, dist, bank_group)
    pipe, stats, state = B.pipe, B.stats, B.state
    z0, ctx_neg, ctx_pos = B.z0, B.ctx_neg, B.ctx_pos
    chunks_per_scene = B.cps
    B0_inflight = B.inflight
    B.keep = {} if (args.dump_outputs and rank == 0) else None
    dt_s, my_views, my_renders = B.run(args.warmup, args.steps)
    if B.keep is not None:                 # before the instrumented steps below overwrite the gradient buffers
        write_outputs(args.dump_outputs, last_step_outputs(B))
        B.keep = None
    g = B.next_step
    if dist is not None:
        tv = torch.tensor([my_views, my_renders], device=dev, dtype=torch.float64)
        dist.all_reduce(tv)
        views_done, renders_done = int(tv[0].item()), int(tv[1].item())
    else:
        views_done, renders_done = my_views, my_renders
    value = views_done / dt_s
    dn_s, rs_s = B.halves()          # this rank's GPU time in the two halves (rank 0 reports; ranks run in lock step)
    step = B.step

    # ---------------------------------------------------------------- --full only: everything below up to the result line
    # ---------------------------------------------------------------- roofline of the dominant kernel (instrumented extra step)
    roof = roof_fp8 = None
    if args.full and args.workload == "edit" and rank == 0:
        roof, _ = denoise_roofline(args, args.dtype, pipe, sdops, z0, ctx_neg, ctx_pos, state["bank"], dev)
        if args.dtype == "fp8":
            roof_fp8, _ = denoise_roofline(args, args.dtype, pipe, sdops, z0, ctx_neg, ctx_pos, state["bank"], dev, fp8_class=True)

    roof_raster = None
    if args.full and rank == 0:
        B.rank0_only = True
        if args.workload == "raster":
            roof = raster_roofline(args, B, g, stats, H * W)
        else:
            rr = raster_roofline(args, B, g, stats, H * W)          # the rasterizer half of the same run: chain roofline at this N
            # headline fraction = priced on the (tile, Gaussian) pairs the kernels really move (tight boxes); `frac_reference_lists` prices
            # the same time against gsplat's longer lists (what the reference would have to move)
            ch = rr["chain"]
            roof_raster = {"bound": "hbm", "unit": "GB/s", "peak": 8000.0, "achieved": round(ch["frac"] * 8000.0, 1),
                           "frac": ch["frac"], "frac_counters": ch["frac_counters"], "frac_8d_unbatched": ch["frac_8d_unbatched"],
                           "kernel_us_per_view": ch["kernel_us_per_view"], "algorithmic_MB_per_view": ch["algorithmic_MB_per_view"],
                           "traffic_MB_per_view": ch["traffic_MB_per_view"], "traffic_ratio": ch.get("traffic_ratio"), "N": ch["N"],
                           "views_per_launch_set": ch["views_per_launch_set"], "M_mean": ch["M_mean"], "M_processed_mean": ch["M_processed_mean"],
                           "formula": ch["formula"], "dominant_stage": rr["kernel"], "dominant_stage_frac": rr["frac"]}

    # ---------------------------------------------------------------- secondary: the f16 activation path (the dtype that meets north_star's 1e-3)
    secondary = None
    if args.full and rank == 0 and world == 1 and args.workload == "edit" and args.dtype == "bf16" and not args.no_secondary:
        del B, pipe, state, z0, step
        torch.cuda.empty_cache()
        B2 = Bench(args, "f16", rank, world, dev, None, None)
        n2 = min(args.steps, B2.cps)           # up to one whole scene, so that the short last chunk and the reference share weigh as in `value`
        t2, v2, _ = B2.run(1, n2)
        secondary = {"dtype": "f16", "value": round(v2 / t2, 4), "unit": "views/s", "steps": n2, "warmup": 1,
                     "note": "same workload with f16 activations (latents within 1e-3 rel of the fp32 oracle, tests/test_fullgeom_gpu.py)"}
        del B2
        torch.cuda.empty_cache()
    # ... and BASELINE configs[3]'s "fp8 MFMA UNet path" on the same workload: e4m3 resnet convolutions (>= 16 x 16 maps) on the block-scaled MFMA
    # (+ with --fp8-linears 7 the transformer linears of the C = 640 / 1280 levels), bf16 elsewhere (latents 2.7e-2 from the fp32 oracle: a
    # reported variant, never `value`).  A failure here must not cost the headline line.
    secondary_fp8 = None
    if args.full and rank == 0 and world == 1 and args.workload == "edit" and args.dtype == "bf16" and not args.no_secondary:
        try:
            B3 = Bench(args, "fp8", rank, world, dev, None, None)
            n3 = min(args.steps, B3.cps)
            t3, v3, _ = B3.run(1, n3)
            r8, _ = denoise_roofline(args, "fp8", B3.pipe, sdops, B3.z0, B3.ctx_neg, B3.ctx_pos, B3.state["bank"], dev, fp8_class=True)
            per_s = (UNET_GFLOP_XVIEW + CN_GFLOP_XVIEW) * 1e9
            pair8 = 2 * per_s - ((UNET_PREFIX_GFLOP + CN_PREFIX_GFLOP) * 1e9 if sdops.OPTIONS.cfg_share else 0.0)
            fl8 = v3 * (nsteps * pair8 + VAE_DECODE_GFLOP * 1e9) + (n3 / B3.cps) * nsteps * 4 * pair8
            secondary_fp8 = {"dtype": "fp8", "value": round(v3 / t3, 4), "unit": "views/s", "steps": n3, "warmup": 1,
                             "roofline": r8,
                             "mfma_util_step_mixed_peak": round(fl8 / t3 / (r8["mixed_peak_tflops"] * 1e12), 4),
                             "mfma_util_step_vs_bf16_peak": round(fl8 / t3 / (PEAK_TFLOPS["bf16"] * 1e12), 4),
                             "config": {"fp8_linears_mask": args.fp8_linears, "fp8_min_hw": args.fp8_min_hw,
                                        "layernorm_fold_and_graph_merges": not args.fp8_linears},
                             "note": ("same workload, --dtype fp8: e4m3 resnet convolutions beside the bf16 transformer blocks with the LayerNorm fold and the "
                                      "round-5 graph merges (latents within 6e-2 rel of the fp32 oracle at every step, measured 2.7e-2 on the predicted curve: "
                                      "tests/test_fullgeom_gpu.py::test_edit_f7_h64_fp8_convs_with_folded_linears)") if not args.fp8_linears else
                                     ("same workload, --dtype fp8 --fp8-linears %d: e4m3 convolutions + C = 640 / 1280 transformer linears, bf16 elsewhere "
                                      "(tests/test_fullgeom_gpu.py::test_edit_f7_h64_fp8_convs_and_linears)" % args.fp8_linears)}
            del B3
        except Exception as ex:                    # noqa: BLE001 -- reported, not raised
            secondary_fp8 = {"dtype": "fp8", "error": f"{type(ex).__name__}: {ex}"[:300]}
        torch.cuda.empty_cache()

    # ---------------------------------------------------------------- CPU baseline (oracle, rank 0, bounded sample)
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args)

    if rank == 0:
        metric = ("edited views/sec @512x512 (ControlNet denoise + splat render+bwd)" if args.workload == "edit" else
                  "raster-only train-render fwd+bwd views/sec @512x512 (BASELINE configs[4])")
        if args.workload == "edit":
            # algorithmic FLOP of the timed region, as executed (reference K/V cached): CFG doubles every chunk frame; the reference
            # trajectory (4 views x 2) is computed once per scene by ONE rank (or by every rank with --ref-mode replicate)
            per_sample = (UNET_GFLOP_XVIEW + CN_GFLOP_XVIEW) * 1e9
            # executed FLOP of a CFG pair: the shared prefix runs once (not on a sample-sharded reference trajectory, which holds other subsets)
            shared = (UNET_PREFIX_GFLOP + CN_PREFIX_GFLOP) * 1e9 if sdops.OPTIONS.cfg_share else 0.0
            pair = 2 * per_sample - shared
            pair_ref = 2 * per_sample - (0.0 if (world > 1 and args.ref_mode == "allgather") else shared)
            scenes = args.steps / chunks_per_scene
            ref_copies = world if args.ref_mode == "replicate" and world > 1 else 1
            flop = views_done * (nsteps * pair + VAE_DECODE_GFLOP * 1e9) + scenes * ref_copies * nsteps * 4 * pair_ref
            mfma_util = flop / dt_s / (world * PEAK_TFLOPS[args.dtype] * 1e12)
            par = (f"views of one scene sharded x{world}" + (" (load balanced: the bank owner edits ~4 views fewer)" if world > 1 and args.ref_mode in ("rotate", "owner0") else " (v % N)") +
                   "; reference bank: " +
                   ({"rotate": "owner rotates per scene, per-DDIM-step async RCCL broadcast", "owner0": "rank 0 owns, per-DDIM-step async RCCL broadcast",
                     "replicate": "replicated on every rank (no collective)",
                     "allgather": "trajectory sharded by sample, per-layer RCCL all-gather of K / V^T"}[args.ref_mode] if world > 1 else "local") +
                   f"; flat async gradient all-reduce; {args.cobatch} chunk(s) per launch set (one network batch), {B0_inflight} launch set(s) in flight on independent "
                   "stream pairs; ControlNet || UNet encoder on 2 HIP streams")
        else:
            flop, mfma_util = None, None
            par = f"every rank renders its own {V} cameras (x{world}); flat async gradient all-reduce"
        out = {"metric": metric, "value": round(value, 4),
               "unit": "views/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(1e3 * dt_s / args.steps, 2), "higher_is_better": True, "scaling": "weak",
               "vs_baseline": None, "dtype": args.dtype if args.workload == "edit" else "f32", "data": "synthetic",
               "config": {"workload": f"{'masked-edit' if args.mask else 'bear-like'} scene, {V} views, ref_view_num=4, chunk_size={c}, "
                                      f"{nsteps} DDIM steps, SD1.5+ControlNet-depth shapes (random weights), "
                                      f"{args.gaussians} Gaussians, 512x512" if args.workload == "edit" else
                                      f"raster-only fwd+bwd (+ fused L1+SSIM loss), {args.gaussians} Gaussians, {V} random cameras/GPU, 512x512, fx=fy=540",
                          "views_per_step": round(views_done / args.steps, 3), "chunks_per_scene_per_rank": chunks_per_scene, "parallelism": par,
                          "chunks_per_launch_set": args.cobatch if args.workload == "edit" else 1,
                          "mean_intersections_M": int(np.mean(stats["M"])) if stats["M"] else 0,
                          "ref_trajectory_in_timed_region": bool(args.workload == "edit"),
                          "cfg_shared_prefix": bool(sdops.OPTIONS.cfg_share) if args.workload == "edit" else None,
                          "layernorm_fold_levels_1_3": (os.environ.get("GC_DN_FOLD_LN", "0" if (args.dtype == "fp8" and args.fp8_linears) else "2") != "0") if args.workload == "edit" else None,
                          "level0_transformer_blocks": ("one-launch head + tail" if sdops.OPTIONS.fused_head and sdops.OPTIONS.fused_tail
                                                        else f"fused_head={sdops.OPTIONS.fused_head} fused_tail={sdops.OPTIONS.fused_tail}") if args.workload == "edit" else None,
                          "ref_trajectory_share_per_step": f"{nsteps}/{chunks_per_scene} DDIM steps of the next scene's 4 reference views" if args.workload == "edit" else None,
                          # the EFFECTIVE switches of this run (defaults = the product configuration; any GC_* experiment variable that changed
                          # one shows up here, so a headline line is provably the default build): sd.ops.KernelOptions + the bench-level toggles
                          "kernel_options": effective_options(sdops, args),
                          "is_product_default": effective_options(sdops, args) == effective_options(None, None)},
               # the two halves separately (GPU time of rank 0's launch stream between HIP events in the timed steps)
               # (the wall time of the timed region is apportioned to the halves by their share of the per-chunk GPU spans: with one
               # chunk in flight that is the measured span itself, with several the spans overlap but their ratio stands)
               "denoise_views_per_s": round(my_views / (dt_s * dn_s / (dn_s + rs_s)), 4) if (args.workload == "edit" and dn_s > 0) else None,
               "raster_fwd_bwd_iters_per_s": round(my_renders / (dt_s * rs_s / (dn_s + rs_s)), 2) if rs_s > 0 else None,
               "halves": {"denoise_s": round(dn_s, 4), "raster_train_s": round(rs_s, 4), "views_rank0": my_views, "train_renders_rank0": my_renders,
                          "spans_overlap": B0_inflight > 1,
                          "note": "spans = GPU time between HIP events on each chunk's launch stream (they overlap when several chunks are in flight; the rates above apportion the wall time by their ratio); denoise half = eval renders + disparity + 20-step denoise + VAE decode + reference share; raster half = training render fwd + L1/SSIM + bwd"},
               "mfma_util_step": None if mfma_util is None else round(mfma_util, 4),
               "algorithmic_tflop_timed_region": None if flop is None else round(flop / 1e12, 1),
               "full": bool(args.full),              # the five fields below are measured with --full only (null otherwise)
               "secondary": secondary, "secondary_fp8": secondary_fp8,
               "roofline": roof, "roofline_raster": roof_raster, "cpu_baseline": cpu}
        if roof_fp8 is not None:          # --dtype fp8: the e4m3 GEMM class against the 5 PF e4m3 peak, and the step against the mixed peak
            out["roofline_fp8"] = roof_fp8
            out["mfma_util_step_mixed_peak"] = round(flop / dt_s / (world * roof_fp8["mixed_peak_tflops"] * 1e12), 4)
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()                      # ranks leave together (with --full rank 0 ran more instrumented steps)
        dist.destroy_process_group()



PEAK_E4M3_TFLOPS = 5000.0      # dense OCP e4m3 on the block-scaled K = 128 MFMA (MI355X_MICROARCH.md: ~5 PF dense, 4 647 TF measured)


def denoise_roofline(args, dtype_name, pipe, sdops, z0, ctx_neg, ctx_pos, bank, dev, fp8_class=False):
    """One instrumented chunk on a single stream, every GEMM / attention / block launch bracketed by HIP events (GemmProfiler).
    Returns (roofline dict, per-class summary).  fp8_class=False: the dominant kernel class of the chunk against the dense 2-byte MFMA peak.
    fp8_class=True (`--dtype fp8` runs): the dominant e4m3 GEMM class against the dense e4m3 peak (5 PF) -- the chunk's dominant kernel stays
    the bf16 attention, reported under `other` with its own fraction of 2.5 PF."""
    c, H, W = args.chunk_size * max(1, args.cobatch), 512, 512          # the instrumented launch set = what the timed steps launch (cobatch chunks)
    prof = GemmProfiler("F16" if dtype_name == "f16" else "BF16")
    for net in (pipe.unet, pipe.controlnet):             # un-padded input channels of the e4m3 convolutions (weights pad Cin to 128)
        for k, v in net.w.items():
            if k.endswith(".w8") and ".resnets." in k and (k[:-2] + "weight") in net.w:
                wt = net.w[k[:-2] + "weight"]                                   # prepared 2-byte weight: Cout x (3 x 3 x Cin), in whatever rank
                prof.true_cin[v.data_ptr()] = int(wt.numel() // (wt.shape[0] * 9))
    two = pipe.two_streams
    pipe.two_streams = False          # HIP events bracket one kernel only when nothing else shares the GPU: single stream here
    disp_i = torch.rand(c, 3, H, W, device=dev)
    torch.cuda.synchronize()
    pipe.edit_chunk_cached(z0[:c], disp_i, ctx_neg, ctx_pos, bank)          # one untimed chunk in the SAME single-stream mode first: the instrumented chunk
    torch.cuda.synchronize()                                               # then starts from that mode's steady state (one run in five read 9 % high without it)
    prof.wrap(sdops)
    try:
        lat = pipe.edit_chunk_cached(z0[:c], disp_i, ctx_neg, ctx_pos, bank)  # noqa: F841
    finally:
        prof.unwrap(sdops)
        pipe.two_streams = two
    sm = prof.summary()
    if os.environ.get("GC_BENCH_SHAPES"):
        tab = {}
        for op, M, N, K, fl, s_, e_ in prof.shapes:
            t = tab.setdefault((op, M, N, K, fl), [0, 0.0]); t[0] += 1; t[1] += s_.elapsed_time(e_)
        for (op, M, N, K, fl), (n, ms) in sorted(tab.items(), key=lambda kv: -kv[1][1]):
            print(f"# shape {op:8s} M={M:6d} N={N:5d} K={K:5d} {fl:40s} x{n:4d} {ms:8.2f} ms {ms / n * 1e3:7.1f} us {2.0 * M * N * K * n / ms / 1e9:7.1f} TF/s", file=sys.stderr)
    is8 = lambda k: k.startswith("gemm8q<e4m3")
    peak_of = lambda k: PEAK_E4M3_TFLOPS if is8(k) else PEAK_TFLOPS[dtype_name]
    cand = {k: v for k, v in sm.items() if is8(k)} if fp8_class else sm
    kind, d = max(cand.items(), key=lambda kv: kv[1]["ms"])
    ach = d["flop"] / (d["ms"] * 1e-3) / 1e12
    # HBM bytes per launch of the dominant kernel from the committed PMC passes (profiles/r0x_attn_traffic.json, scripts/
    # pmc_kernel_traffic.py: FETCH_SIZE / WRITE_SIZE in separate rocprofv3 passes on the UNet's 5-set launch at chunk_size 3)
    traffic = None
    traffic_src = None
    for tname in ("r05_attn_traffic.json", "r04_attn_traffic.json", "r02_attn_traffic.json"):
        tpath = os.path.join(ROOT, "profiles", tname)
        if kind.startswith(("k_attn4", "k_attn5")) and c == 3 and os.path.exists(tpath) and traffic is None:
            for kn, v in json.load(open(tpath))["kernels"].items():
                if kind[:7] in kn and "traffic_MB_per_dispatch" in v:
                    traffic = int(round(v["traffic_MB_per_dispatch"] * 1e6))
                    traffic_src = f"profiles/{tname}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over this kernel (not measured in this run)"
    desc = (" (multi-K/V-set flash attention, dn_attn.hip)" if kind.startswith("k_attn") else "" if is8(kind) else
            " (k_gemm / k_gemm8 MFMA GEMM and implicit 3x3 conv, variant picked per grid, dn_gemm.hip)")
    roof = {"bound": "mfma", "kernel": kind + desc,
            "achieved": round(ach, 2), "peak": peak_of(kind), "unit": "TFLOP/s",
            "frac": round(ach / peak_of(kind), 4), "traffic": traffic, "traffic_source": traffic_src,
            "launches": d["launches"], "avg_launch_us": round(1e3 * d["ms"] / d["launches"], 2),
            "algorithmic_gflop_per_launch": round(d["flop"] / d["launches"] / 1e9, 3),
            "other": {k: {"launches": v["launches"], "ms": round(v["ms"], 2),
                          "tflops": round(v["flop"] / (v["ms"] * 1e-3) / 1e12, 2), "frac_of_its_peak": round(v["flop"] / (v["ms"] * 1e-3) / 1e12 / peak_of(k), 4)}
                      for k, v in sm.items() if k != kind}}
    if kind.startswith("k_attn"):
        # the dominant kernel's launches of the instrumented set by size.  rocprofv3's per-kernel average covers EVERY launch of a run (full launch sets,
        # the 2-chunk set that ends a scene, the 8- / 4-frame reference trajectories), so it is lower than avg_launch_us above whenever the sets are larger
        # than a trajectory batch: compare per workgroup count (`python scripts/rocpd_stats.py <db> 70 k_attn5` prints the same groups from the trace)
        groups = {}
        for nm, fr, lq, ns, s_, e_ in prof.att_kinds:
            if nm != kind:
                continue
            g_ = groups.setdefault((fr, lq, ns), [0, 0.0]); g_[0] += 1; g_[1] += s_.elapsed_time(e_)
        roof["rocprofv3_note"] = ("avg_launch_us / launch_kinds are single-stream HIP-event durations of ONE full launch set; a rocprofv3 trace of this command averages every "
                                  "k_attn5 launch of the run (2-chunk sets, 8- / 4-frame reference trajectories: smaller) and times them while a second launch set shares "
                                  "the GPU (--inflight 2: longer) -- compare per workgroup count with the trace of `bench.py --full --inflight 1` "
                                  "(profiles/r06_bench_kernel_stats_bf16_single_stream.txt: 2 717 us in the trace vs 2 724 us live for the 3 072-workgroup launches; `scripts/rocpd_stats.py <db> 70 k_attn5`)")
        roof["launch_kinds"] = [{"frames": fr, "queries_per_frame": lq, "kv_sets": ns, "workgroups": fr * 8 * max(1, lq // 256), "launches": n_,
                                 "avg_us": round(1e3 * ms_ / n_, 1)} for (fr, lq, ns), (n_, ms_) in sorted(groups.items(), reverse=True)]
    # share of the instrumented chunk's algorithmic FLOP that runs on e4m3 operands -> the mixed peak a whole-step utilisation is priced against:
    # peak_mixed = 1 / (f8 / 5 PF + (1 - f8) / 2.5 PF) (time to run each share at its own dense peak)
    f_tot = sum(v["flop"] for v in sm.values())
    f8 = sum(v["flop"] for k, v in sm.items() if is8(k)) / max(f_tot, 1.0)
    roof["e4m3_flop_share_of_instrumented_chunk"] = round(f8, 4)
    roof["mixed_peak_tflops"] = round(1.0 / (f8 / PEAK_E4M3_TFLOPS + (1.0 - f8) / PEAK_TFLOPS[dtype_name]), 1)
    return roof, sm


class LibTimer:
    """Proxy of the ctypes library handle that brackets every compute entry point with HIP events on the launch stream
    (instrumented pass of the raster-only workload)."""
    SKIP = ("gc_last_error_string", "gc_abi_version", "gc_raster_read_count")

    def __init__(self, lib):
        self._l = lib
        self.rec = []

    def __getattr__(self, name):
        f = getattr(self._l, name)
        if not name.startswith("gc_") or name.endswith("_bytes") or name in self.SKIP:
            return f

        def timed(*a):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = f(*a)
            e.record()
            self.rec.append((name, s, e))
            return r
        return timed


# algorithmic HBM bytes of one training render (forward + backward) per stage: coefficients of (N Gaussians, M tile
# intersections, HW pixels) from SURVEY.md 8(d), which add up to N*868 + M*124 + HW*44 -- except k_project_sh_bwd: since round 2 it takes
# the forward colours instead of re-reading the 192-byte SH record (reads 108 B, writes 236 B per Gaussian: 344 instead of 552), so the
# chain total is N*660 + M*124 + HW*44 for ONE camera per launch set.
# A batch of C cameras (round 5) reads / writes the camera-independent part of a Gaussian's record once per BATCH: projection
# forward 236 + C * 60 bytes per Gaussian (C * 296 unbatched; the 8d row's 280 + the 16 bytes of depth-sort pair and opacity it writes since
# round 5), projection backward 56 + C * 64 read + 236 written (C * 344 unbatched... 8d: 344).  `raster_stage_bytes` returns the bytes ONE view
# is charged: the batch-aware count is what a launch really has to move, the 8d count what C unbatched renders would.
RASTER_STAGES = {
    # name: (label, per-Gaussian bytes per view [8d], per-Gaussian bytes per BATCH, per-Gaussian bytes per view inside a batch, per pair, per pixel)
    "gc_project_sh_fwd": ("k_project_sh_fwd", 280, 236, 60, 0, 0),
    "gc_raster_depth_order": ("binning: depth keys + 4 radix passes + scan (raster_sort.hip)", 0, 0, 0, 0, 0),      # counted with the next row
    "gc_raster_bin_tiles_dev": ("binning: emit + 2 tile radix passes + bins (raster_sort.hip)", 0, 0, 0, 44, 0),
    "gc_raster_bin_tiles": ("binning: emit + 2 tile radix passes + bins (raster_sort.hip)", 0, 0, 0, 44, 0),
    "gc_rasterize_fwd": ("k_rasterize_fwd", 0, 0, 0, 40, 20),
    "gc_raster_finalize": ("k_raster_finalize", 0, 0, 0, 0, 0),
    "gc_l1_ssim_fwd_bwd": ("k_ssim_stats + k_ssim_grad (loss, not in the 8d byte count)", 0, 0, 0, 0, 0),
    "gc_rasterize_bwd": ("k_rasterize_bwd", 36, 0, 36, 40, 24),
    "gc_project_sh_bwd": ("k_project_sh_bwd", 344, 56 + 236, 64, 0, 0),
}


def raster_stage_bytes(name, N, M, HW, C=1):
    """(bytes per view by the SURVEY 8d formula, bytes per view when C cameras share a launch set)"""
    _, n8d, n_batch, n_view, cm, chw = RASTER_STAGES[name]
    b8d = n8d * N + cm * M + chw * HW
    if C <= 1:
        return b8d, b8d
    return b8d, (n_batch / C + n_view) * N + cm * M + chw * HW


def raster_roofline(args, B, g, stats, HW):
    """One instrumented step of the raster-only workload: per-stage HIP-event durations -> achieved algorithmic GB/s per stage
    and for the whole forward + backward chain; `traffic` = HBM bytes per launch from the committed rocprofv3 PMC passes
    (profiles/r02_raster_traffic.json, FETCH_SIZE / WRITE_SIZE collected in separate passes by scripts/pmc_traffic.py) when the
    configuration matches, else null."""
    from gaussctrl_amd import _lib as L
    real = L.lib()
    timer = LibTimer(real)
    n_dev = len(stats["dev"])
    r_before = B.state["renders_done"]
    L._lib = timer
    try:
        if args.workload == "raster":
            B.step(g)
        else:                      # default workload: only the training renders of one chunk (fwd + loss + bwd), no denoise
            keep, B.edit = B.edit, False
            try:
                B.step(B.groups(0, B.cobatch)[0])          # one launch set, as the timed steps run them (cobatch chunks)
            finally:
                B.edit = keep
        torch.cuda.synchronize()
    finally:
        L._lib = real
    Ms = [int(v) for a, _ in stats["dev"][n_dev:] for v in a.reshape(-1).cpu()] or stats["M"][-8:]        # pairs the instrumented views really binned (tight boxes)
    nviews = max(1, B.state["renders_done"] - r_before)            # training renders of the instrumented step (a batched call covers several)
    M_proc = float(np.mean(Ms))
    # The SURVEY 8d byte formula counts the intersections of the reference's lists (gsplat's 3-sigma boxes): that M is measured here on
    # the same cameras with the tight boxes switched off (untimed); `frac` prices the chain against it, `frac_processed_pairs` against
    # the shorter lists the product path really moves.
    scene, j = divmod(g - g % B.cps if args.workload != "raster" else g, B.cps)
    Mg = []
    for i in B.chunks_of(scene)[j]:
        auxg = B.gops.RenderAux(); auxg.tight_boxes = False
        with torch.no_grad():
            p_ = B.params
            B.gops.render_view(p_["means"], p_["scales"], p_["quats"], p_["opacities"], p_["features_dc"], p_["features_rest"], B.cams[i],
                               B.bg, False, 3, auxg)
        Mg.append(int(auxg.M))
    M = float(np.mean(Mg)) if Mg else M_proc
    N = args.gaussians
    per = {}
    alias = {"gc_rasterize_bwd_clamped": "gc_rasterize_bwd", "gc_raster_finalize_into": "gc_raster_finalize",          # same kernels, round-3 entry points
             "gc_project_sh_fwd_boxes": "gc_project_sh_fwd", "gc_raster_bin_tiles_boxes": "gc_raster_bin_tiles_dev",
             # round 5: the batched-views entry points (one call covers every view of the step: per-view time = call time / views)
             "gc_project_sh_fwd_views": "gc_project_sh_fwd", "gc_raster_depth_order_views": "gc_raster_depth_order",
             "gc_raster_bin_tiles_views": "gc_raster_bin_tiles_dev", "gc_rasterize_fwd_views": "gc_rasterize_fwd",
             "gc_rasterize_bwd_views": "gc_rasterize_bwd", "gc_project_sh_bwd_views": "gc_project_sh_bwd",
             "gc_l1_ssim_fwd_bwd_views": "gc_l1_ssim_fwd_bwd",
             # round 6: the gather-free chain
             "gc_raster_order_boxes_views": "gc_raster_depth_order", "gc_raster_bin_sorted_views": "gc_raster_bin_tiles_dev"}
    tot_stage = {}
    for name, s, e in timer.rec:
        k = alias.get(name, name)
        tot_stage[k] = tot_stage.get(k, 0.0) + s.elapsed_time(e) * 1e-3
    per = {k: [v / nviews] for k, v in tot_stage.items()}            # seconds per training view and stage
    traffic = None
    # PMC traffic of the configuration that ran: the batched-views passes (round 5, 8 views per launch set) or the one-camera-per-launch ones
    batched = B.view_batch and nviews >= 2
    Cb = nviews if batched else 1                   # every view of the instrumented launch set goes through ONE batched call
    # (the round-5 passes were taken on the pair chain: they describe this run only with GC_RASTER_SORTED_BOXES=0)
    names = ((f"r06_raster_traffic_views{Cb}.json",) + (() if B.sorted_boxes else (f"r05_raster_traffic_views{Cb}.json",))) if batched else ("r03_raster_traffic.json", "r02_raster_traffic.json")
    for tname in names:
        tpath = os.path.join(ROOT, "profiles", tname)
        if traffic is None and os.path.exists(tpath):
            traffic = json.load(open(tpath)).get(str(N))
    C = Cb                                                           # cameras per launch set of the instrumented step
    stages, tot_8d, tot_b, tot_s = {}, 0.0, 0.0, 0.0
    for name in RASTER_STAGES:
        if name not in per:
            continue
        label = RASTER_STAGES[name][0]
        secs = float(np.mean(per[name]))
        b8d, b = raster_stage_bytes(name, N, M_proc, HW, C)           # priced on the pairs the kernels really bin (tight boxes)
        b8d_ref = raster_stage_bytes(name, N, M, HW, 1)[0]            # ... and the 8d formula on gsplat's longer lists (what the reference would move)
        tot_8d += b8d_ref; tot_b += b; tot_s += secs
        tr = None if not traffic or name not in traffic else traffic[name]
        stages[name] = {"kernel": label, "avg_us": round(secs * 1e6, 1), "algorithmic_MB": round(b / 1e6, 1),
                        "GBps": round(b / secs / 1e9, 1) if b else None, "algorithmic_MB_8d_unbatched": round(b8d_ref / 1e6, 1),
                        "traffic_MB": tr, "traffic_GBps": None if tr is None else round(tr * 1e6 / secs / 1e9, 1)}
    traffic_ratio = traffic_MB = frac_counters = None
    if traffic:                   # counters of the committed PMC passes at this N: what the chain really moved, over the same stages
        traffic_MB = sum(v for k, v in traffic.items() if k in stages or k == "loss+finalize")
        traffic_ratio = round(traffic_MB * 1e6 / tot_b, 3)
        frac_counters = round(traffic_MB * 1e6 / tot_s / 8e12, 4)
    dom = max((k for k in stages if stages[k]["GBps"]), key=lambda k: stages[k]["avg_us"])
    d = stages[dom]
    ach = d["algorithmic_MB"] * 1e6 / (d["avg_us"] * 1e-6) / 1e9
    assert all(v["GBps"] is None or v["GBps"] <= 8000.0 for v in stages.values()), "a stage priced above the HBM peak: its byte count is wrong"
    return {"bound": "hbm", "kernel": f"{d['kernel']} ({dom}, dominant stage of the render fwd+bwd chain)", "achieved": round(ach, 1),
            "peak": 8000.0, "unit": "GB/s", "frac": round(ach / 8000.0, 4), "traffic": d["traffic_MB"] and d["traffic_MB"] * 1e6,
            "avg_launch_us": d["avg_us"], "algorithmic_bytes_per_launch": d["algorithmic_MB"] * 1e6,
            "chain": {"algorithmic_MB_per_view": round(tot_b / 1e6, 1), "kernel_us_per_view": round(tot_s * 1e6, 1),
                      "GBps": round(tot_b / tot_s / 1e9, 1),
                      # three readings of the same time, most conservative first:
                      #   frac                -- batch-aware algorithmic bytes on the pairs really binned (what one launch set has to move) / time
                      #   frac_counters       -- HBM bytes the PMC counters saw (committed passes at this N and batch) / time
                      #   frac_8d_unbatched   -- SURVEY 8d's per-view formula on gsplat's lists (what C unbatched reference renders would move) / time
                      "frac": round(tot_b / tot_s / 8e12, 4), "frac_counters": frac_counters, "frac_8d_unbatched": round(tot_8d / tot_s / 8e12, 4),
                      "traffic_MB_per_view": None if traffic_MB is None else round(traffic_MB, 1),
                      "views_in_sample": nviews, "views_per_launch_set": C,
                      "N": N, "M_mean": int(M), "M_processed_mean": int(M_proc),
                      "traffic_ratio": traffic_ratio,
                      "formula": ("per view of a C-camera launch set: N*((236+56+236)/C + 60+36+64) + M*124 + HW*44 bytes (DESIGN.md 3.1; C = 1 gives SURVEY.md 8d's "
                                  "N*660 + M*124 + HW*44 plus the 32 bytes of sort pair / opacity written since round 5); M = pairs binned on the tight boxes "
                                  "(M_processed_mean); M_mean = intersections of gsplat's boxes, used only by frac_8d_unbatched")},
            "stages": stages}


def cpu_baseline(args):
    """Oracle ("port") timed on the host cores on a BOUNDED sample of the same workload.
    Denoise: ONE real CFG ControlNet+UNet cross-view step at the reference's CPU-runnable shape (configs[0]: chunk_size 1 ->
    f = 4 references + 1 = 5 frames, CFG batch 10) on the full 64 x 64 latents, fp32 torch on every core; an edited view at
    chunk_size 1 costs the whole f = 5 batch for 20 such steps.  Rasterizer: the C oracle (OpenMP build of oracle/raster_ref.c,
    every core; the sort is serial) at the run's full N: one eval render + one training render fwd + bwd.  VAE decode: one frame."""
    from oracle import raster_c, sd15_torch as sd
    from gaussctrl_amd import synthetic as syn
    cores = os.cpu_count() or 1
    # Threads: measured on the GPU box (256 logical cores, round 5, profiles/r05_bench_bf16_start.json): fp32 torch on ALL 256 logical cores takes
    # 289 s for the one denoise step that 64 threads finish in ~30 s (oneDNN / OpenMP oversubscription of the SMT siblings and NUMA domains) --
    # "every core" makes the baseline 10x WORSE and the default run 5 minutes longer.  The line therefore states the thread count that was used
    # (`cores` = 64, both for torch and for the OpenMP rasterizer), which is the faster of the two configurations measured.
    threads = min(cores, 64)
    torch.set_num_threads(threads)
    os.environ["OMP_NUM_THREADS"] = str(threads)
    raster_c.use_threads(True)
    try:
        N = args.gaussians
        P = syn.make_gaussians(N, seed=0)
        c2w = syn.make_cameras(1, seed=1)[0]
        K = syn.ROUND_INTRINSICS if args.workload == "raster" else syn.BEAR_INTRINSICS
        bgc = np.zeros(3, np.float32)
        v_rgb = np.ones((512, 512, 3), np.float32)
        t0 = time.perf_counter()
        if args.workload != "raster":
            raster_c.render(P, c2w, K["fx"], K["fy"], K["cx"], K["cy"], 512, 512, bgc, training=False)
        raster_c.render(P, c2w, K["fx"], K["fy"], K["cx"], K["cy"], 512, 512, bgc, training=True, v_rgb=v_rgb)
        t_raster = time.perf_counter() - t0
    finally:
        raster_c.use_threads(False)
    if args.workload == "raster":
        return {"value": round(1.0 / t_raster, 4), "unit": "views/s", "cores": threads, "kind": "port",
                "sample": f"C oracle (oracle/raster_ref.c, OpenMP build, {threads} threads of the box's {cores} logical cores; serial sort) one training render fwd+bwd at the full "
                          f"N={N}: {t_raster:.2f}s per view"}
    sd.ATTN_IMPL = "sdpa"                    # the fused CPU attention (the explicit form needs 5 x [80,4096,4096] fp32 tensors per layer)
    with torch.no_grad():
        uw = sd.make_unet_weights(sd.SD15, 100); cw = sd.make_controlnet_weights(sd.SD15, 200)
        f = 5
        lat = torch.randn(f, 4, 64, 64); disp = torch.rand(f, 3, 512, 512)
        cn, cp = torch.randn(1, 77, 768), torch.randn(1, 77, 768)
        wl = torch.randn(f, 4, 16, 16); wd = torch.rand(f, 3, 128, 128)
        sd.denoise_chunk(uw, cw, wl, wd, cn, cp, 5.0, 1, sd.SD15, 20)      # untimed warm-up (thread pool, oneDNN primitives) on a 16 x 16 latent
        t0 = time.perf_counter()
        sd.denoise_chunk(uw, cw, lat, disp, cn, cp, 5.0, 1, sd.SD15, 20)
        t_step = time.perf_counter() - t0
        del uw, cw
        vw = sd.make_vae_decoder_weights(sd.VAE_SD, 300)
        t0 = time.perf_counter()
        sd.vae_decode(vw, torch.randn(1, 4, 64, 64), sd.VAE_SD)
        t_vae = time.perf_counter() - t0
        del vw
    per_view = 20 * t_step + t_vae + t_raster
    return {"value": round(1.0 / per_view, 6), "unit": "views/s", "cores": threads, "kind": "port",
            "sample": f"fp32 torch on {threads} threads of the box's {cores} logical cores (all 256 measured 10x slower, see bench.py; one untimed warm-up step on a 16x16 latent first): 1 of 20 CFG ControlNet+UNet cross-view steps, f=5 (CFG batch 10) on the full 64x64 latents = {t_step:.1f}s (x20 per "
                      f"edited view at chunk_size 1); VAE decode of one frame = {t_vae:.1f}s; C rasterizer (OpenMP, {threads} threads) eval + "
                      f"train fwd+bwd at N={N} = {t_raster:.2f}s"}


if __name__ == "__main__":
    main()
