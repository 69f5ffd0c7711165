"""One densifying refinement at N = 1 M (about 5 % split, 5 % duplicated, 5 % culled): the HIP kernels of csrc/train_refine.hip against the
same step written with torch indexing and `cat` (what gc_trainer.CullCallback and nerfstudio's refinement_after do), in one process on the
same inputs.  5 warm-up + 20 timed repetitions each, device-synchronised (events around every repetition, median and min reported).

    python scripts/bench_refine.py [--n 1000000] [--out profiles/refine_bench.txt]

Needs a GPU: without one it fails and writes nothing."""
import argparse
import ctypes as C
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussctrl_amd import _lib as L  # noqa: E402

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
TH = dict(max_dim=512.0, grad=0.0002, size=0.01, alpha=0.1, scale=0.5, split_screen=0.05, cull_screen=0.15)
NS = 2


def make_scene(N, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = {"means": torch.randn(N, 3, generator=g), "quats": torch.randn(N, 4, generator=g), "features_dc": torch.randn(N, 3, generator=g),
         "features_rest": torch.randn(N, 15, 3, generator=g) * 0.1}
    u = torch.rand(N, generator=g)
    # 5 % big + high (split), 5 % small + high (dup), 5 % transparent (culled), the rest quiet
    smax = torch.where(u < 0.05, torch.tensor(0.03), torch.tensor(0.004))
    high = u < 0.10
    alpha = torch.where((u >= 0.10) & (u < 0.15), torch.tensor(0.04), torch.tensor(0.6))
    P["scales"] = torch.log(smax[:, None] * (torch.rand(N, 3, generator=g) * 0.5 + 0.5))
    P["scales"][:, 0] = torch.log(smax)
    P["opacities"] = torch.logit(alpha)[:, None]
    cnt = torch.full((N,), 3.0)
    avg = torch.where(high, torch.tensor(0.002), torch.tensor(0.00005))
    stats = [(avg * cnt / (0.5 * TH["max_dim"])), cnt, torch.full((N,), 0.01)]
    P = {k: P[k].to(dev).contiguous() for k in NAMES}
    mom = [{k: torch.randn_like(v) * 1e-3 for k, v in P.items()}, {k: torch.rand_like(v) * 1e-6 for k, v in P.items()}]
    return P, [t.to(dev) for t in stats], mom


def hip_step(P, stats, mom, samples_full):
    """plan -> read-back -> apply; returns (outputs, counts, (plan event pair), (apply event pair))"""
    lib = L.lib()
    N = P["means"].shape[0]
    dev = P["means"].device
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    action = torch.empty(N, dtype=torch.int32, device=dev); ranks = torch.empty(3, N, dtype=torch.int32, device=dev)
    counts = torch.zeros(5, dtype=torch.int32, device=dev)
    nb = lib.gc_refine_plan_workspace_bytes(L.i64(N))
    ws = torch.empty(nb // 4 + 1, dtype=torch.int32, device=dev)
    ev[0].record()
    L.check(lib.gc_refine_plan(L.i64(N), L.ptr(P["scales"]), L.ptr(P["opacities"]), L.ptr(stats[0]), L.ptr(stats[1]), L.ptr(stats[2]), L.i32(1),
                               L.i32(NS), L.f32(TH["max_dim"]), L.f32(TH["grad"]), L.f32(TH["size"]), L.i32(1), L.f32(TH["split_screen"]),
                               L.f32(TH["alpha"]), L.i32(1), L.f32(TH["scale"]), L.i32(1), L.f32(TH["cull_screen"]), L.ptr(action), L.ptr(ranks),
                               L.ptr(counts), L.ptr(ws), C.c_size_t(nb), L.stream_ptr()), "gc_refine_plan")
    ev[1].record()
    n_surv, n_split, n_dup, n_out, _ = (int(v) for v in counts.cpu())
    samples = samples_full[:NS * n_split]
    arr = lambda ts: (C.c_void_p * 6)(*[t.data_ptr() for t in ts])
    ins = [[P[k] for k in NAMES], [mom[0][k] for k in NAMES], [mom[1][k] for k in NAMES]]
    outs = [[torch.empty((n_out,) + tuple(t.shape[1:]), device=dev) for t in ts] for ts in ins]
    ev[2].record()
    L.check(lib.gc_refine_apply(L.i64(N), L.i32(NS), L.i32(45), L.i64(n_surv), L.i64(n_split), L.i64(n_dup), L.ptr(action), L.ptr(ranks),
                                L.ptr(samples), arr(ins[0]), arr(ins[1]), arr(ins[2]), arr(outs[0]), arr(outs[1]), arr(outs[2]), L.stream_ptr()),
            "gc_refine_apply")
    ev[3].record()
    return outs, (n_surv, n_split, n_dup, n_out), ev


def torch_step(P, stats, mom, samples_full):
    """the same refinement with boolean indexing and cat, tensor by tensor (nerfstudio's split_gaussians / dup_gaussians / cull_gaussians and
    their dup_in_optim / remove_from_optim)"""
    smax = P["scales"].exp().max(dim=-1).values
    avg = stats[0] / stats[1] * 0.5 * TH["max_dim"]
    high = avg > TH["grad"]
    big = smax > TH["size"]
    split = (big | (stats[2] > TH["split_screen"])) & high
    dup = ~big & high
    below = (torch.sigmoid(P["opacities"]) < TH["alpha"]).squeeze(-1)
    too_big = smax > TH["scale"]
    on_screen = stats[2] > TH["cull_screen"]
    keep = ~split & ~below & ~too_big & ~on_screen
    child_big = (P["scales"] - math.log(1.6)).exp().max(dim=-1).values > TH["scale"]
    es = split & ~below & ~child_big
    ed = dup & ~below & ~too_big
    n_split = int(es.sum())
    samples = samples_full[:NS * n_split]
    q = P["quats"][es] / P["quats"][es].norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3).repeat(NS, 1, 1)
    child_means = torch.bmm(R, (P["scales"][es].exp().repeat(NS, 1) * samples)[..., None])[..., 0] + P["means"][es].repeat(NS, 1)
    outs = [[], [], []]
    for k in NAMES:
        rep = (NS,) + (1,) * (P[k].dim() - 1)
        sp = child_means if k == "means" else (P[k][es] - math.log(1.6)).repeat(rep) if k == "scales" else P[k][es].repeat(rep)
        outs[0].append(torch.cat([P[k][keep], sp, P[k][ed]], 0))
        for j in (0, 1):
            mk = mom[j][k]
            outs[1 + j].append(torch.cat([mk[keep], torch.zeros((sp.shape[0] + int(ed.sum()),) + tuple(mk.shape[1:]), device=mk.device)], 0))
    return outs


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine.py needs a GPU (nothing written)")
    dev = "cuda:0"
    P, stats, mom = make_scene(a.n, dev)
    samples = torch.randn(NS * a.n, 3, device=dev)
    hip_med, hip_min, (outs, cnts, _) = timed(lambda: hip_step(P, stats, mom, samples))
    t_med, t_min, touts = timed(lambda: torch_step(P, stats, mom, samples))
    same = all(o.shape == t.shape for os_, ts_ in zip(outs, touts) for o, t in zip(os_, ts_))
    exact = all(torch.equal(o, t) for k, (o, t) in enumerate(zip(outs[0], touts[0])) if NAMES[k] not in ("means", "scales"))
    # kernel-only times from the events inside hip_step
    plan_ms, apply_ms = [], []
    for _ in range(20):
        _, _, ev = hip_step(P, stats, mom, samples)
        torch.cuda.synchronize()
        plan_ms.append(ev[0].elapsed_time(ev[1])); apply_ms.append(ev[2].elapsed_time(ev[3]))
    plan_ms.sort(); apply_ms.sort()
    n_surv, n_split, n_dup, n_out = cnts
    apply_bytes = 4 * (a.n * (59 * 3 + 4) + n_out * 59 * 3 + NS * n_split * 3)       # records + action/ranks in, rows out, samples
    rate = apply_bytes / (apply_ms[10] * 1e-3)
    lines = [
        f"bench_refine: N = {a.n}, n_split_samples = {NS}; survivors {n_surv}, split sources {n_split}, dup sources {n_dup}, n_out {n_out}",
        f"device: {torch.cuda.get_device_name(0)}; 5 warm-up + 20 timed repetitions, events, device-synchronised",
        f"HIP   refinement (plan + 20-byte read-back + allocation + apply): median {hip_med:.3f} ms, min {hip_min:.3f} ms",
        f"torch refinement (boolean indexing + cat, 18 tensors):            median {t_med:.3f} ms, min {t_min:.3f} ms",
        f"ratio torch / HIP (medians): {t_med / hip_med:.2f}",
        f"gc_refine_plan  (3 launches): median {plan_ms[10]:.3f} ms",
        f"gc_refine_apply (1 launch):   median {apply_ms[10]:.3f} ms, {apply_bytes / 1e6:.1f} MB algorithmic -> {rate / 1e12:.2f} TB/s = "
        f"{100 * rate / 8e12:.1f} % of the 8 TB/s peak",
        f"outputs: shapes equal {same}; copied tensors (quats, opacities, features) bit-identical to the torch step {exact}",
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
