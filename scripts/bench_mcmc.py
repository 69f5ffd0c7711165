"""The MCMC densification kernels at N = 1 M (csrc/train_mcmc.hip): the per-step noise injection `gc_mcmc_inject_noise` against the same update
written in torch (normalise the quaternions, build R, R S^2 R^T, einsum, gate, add), in one process on the same inputs, ALTERNATING; one
relocation of 5 % dead rows and one 5 % growth through gaussctrl_amd.mcmc.  5 warm-up + 20 timed repetitions each, device events around every
repetition, median and min reported.

    python scripts/bench_mcmc.py [--n 1000000] [--out profiles/mcmc_bench.txt]

The one condition: the fused kernel's median must not exceed the torch composition's (exit status 1 otherwise).
Needs a GPU: without one it fails and writes nothing."""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gaussctrl_amd import _lib as L, mcmc  # noqa: E402

NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
HBM_PEAK = 8.0e12               # bytes/s, spec; about 6.3e12 is what a streaming copy achieves on this chip
HBM_COPY = 6.3e12
NOISE_BYTES = 68                # per Gaussian: means 12 + scales 12 + quats 16 + opacity 4 + noise 12 read, means 12 written


def make_scene(N, dev, dead_frac, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    P = {"means": torch.randn(N, 3, generator=g), "quats": torch.randn(N, 4, generator=g), "features_dc": torch.randn(N, 3, generator=g),
         "features_rest": torch.randn(N, 15, 3, generator=g) * 0.1, "scales": torch.log(torch.rand(N, 3, generator=g) * 0.03 + 0.002)}
    alpha = torch.rand(N, generator=g) * 0.79 + 0.01           # 0.01 .. 0.8: every gate is non-zero, every lane moves its 68 bytes
    alpha[torch.rand(N, generator=g) < dead_frac] = 0.002      # dead: sigmoid <= 0.005
    P["opacities"] = torch.logit(alpha)[:, None]
    return {k: P[k].to(dev).contiguous() for k in NAMES}


def hip_noise(P, means, noise, scaler):
    L.check(L.lib().gc_mcmc_inject_noise(L.i64(means.shape[0]), L.ptr(means), L.ptr(P["scales"]), L.ptr(P["quats"]), L.ptr(P["opacities"]),
                                         L.ptr(noise), L.f32(scaler), L.stream_ptr()), "gc_mcmc_inject_noise")


def torch_noise(P, means, noise, scaler):
    q = P["quats"] / P["quats"].norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    cov = (R * torch.exp(2 * P["scales"])[:, None, :]) @ R.transpose(1, 2)
    o = torch.sigmoid(P["opacities"])
    g = 1 / (1 + torch.exp(100 * (o - 0.005)))
    means.add_(torch.einsum("nij,nj->ni", cov, noise) * g * scaler)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0]


class Scene(torch.nn.Module):
    """what gaussctrl_amd.mcmc needs of a model: the six parameters, their param groups and the config"""

    def __init__(self, P, cap):
        super().__init__()
        for k, v in P.items():
            setattr(self, k, torch.nn.Parameter(v.clone()))
        self.config = types.SimpleNamespace(mcmc_min_opacity=0.005, mcmc_cap_max=cap, mcmc_noise_lr=5e5)

    def get_param_groups(self):
        return {"xyz": [self.means], "features_dc": [self.features_dc], "features_rest": [self.features_rest], "opacity": [self.opacities],
                "scaling": [self.scales], "rotation": [self.quats]}


def stepped_scene(P, cap):
    """a Scene with Adam moments for all six tensors (one fused step on small random gradients)"""
    from gaussctrl_amd.train_ops import FusedAdam
    model = Scene(P, cap)
    opts = {g: FusedAdam(ps, lr=1e-9) for g, ps in model.get_param_groups().items()}
    for o in opts.values():
        for p in o.param_groups[0]["params"]:
            p.grad = torch.randn_like(p) * 1e-3
        o.step()
        o.zero_grad(set_to_none=True)
    return model, opts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcmc_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcmc.py needs a GPU (nothing written)")
    dev = "cuda:0"
    N = a.n
    warm, reps = 5, 20
    # ---- noise: the fused kernel and the torch composition on the same inputs, alternating
    P = make_scene(N, dev, 0.0)
    noise = torch.randn(N, 3, device=dev)
    scaler = 1.6e-4 * 5e5
    m_hip, m_torch = P["means"].clone(), P["means"].clone()
    hip_noise(P, m_hip, noise, scaler); torch_noise(P, m_torch, noise, scaler)
    torch.cuda.synchronize()
    diff = float((m_hip - m_torch).abs().max()); moved = float((m_hip - P["means"]).abs().max())
    t_hip, t_torch = [], []
    for k in range(warm + reps):
        h = event_ms(lambda: hip_noise(P, m_hip, noise, scaler))
        t = event_ms(lambda: torch_noise(P, m_torch, noise, scaler))
        if k >= warm:
            t_hip.append(h); t_torch.append(t)
    (hip_med, hip_min), (torch_med, torch_min) = stats(t_hip), stats(t_torch)
    rate = NOISE_BYTES * N / (hip_med * 1e-3)
    # ---- one relocation of 5 % dead rows (dead test + 8-byte read-back + multinomial + relocate), the scene restored before every repetition
    P5 = make_scene(N, dev, 0.05, seed=1)
    model, opts = stepped_scene(P5, cap=N)
    saved = [(p, p.detach().clone()) for p in model.parameters()]
    t_rel, n_rel = [], 0
    for k in range(warm + reps):
        with torch.no_grad():
            for p, v in saved:
                p.data.copy_(v)
        box = {}
        ms = event_ms(lambda: box.update(n=mcmc.relocate(model, opts)))
        n_rel = box["n"]
        if k >= warm:
            t_rel.append(ms)
    # ---- one 5 % growth (weights + read-back + multinomial + N + n_new-row tensors + relocate), from a fresh N-row scene every repetition
    t_add, n_add = [], 0
    for k in range(warm + reps):
        model, opts = stepped_scene(P5, cap=2 * N)
        torch.cuda.synchronize()
        box = {}
        ms = event_ms(lambda: box.update(n=mcmc.add_new(model, opts)))
        n_add = box["n"]
        if k >= warm:
            t_add.append(ms)
    (rel_med, rel_min), (add_med, add_min) = stats(t_rel), stats(t_add)
    ok = hip_med <= torch_med
    lines = [
        f"bench_mcmc: N = {N}, features_rest 45 floats, Adam moments on all six tensors",
        f"device: {torch.cuda.get_device_name(0)}; {warm} warm-up + {reps} timed repetitions, device events, alternating where two are compared",
        f"gc_mcmc_inject_noise (1 launch):              median {hip_med * 1e3:.1f} us, min {hip_min * 1e3:.1f} us",
        f"torch composition (R, R S^2 R^T, einsum, ...): median {torch_med * 1e3:.1f} us, min {torch_min * 1e3:.1f} us",
        f"ratio torch / HIP (medians): {torch_med / hip_med:.1f}   condition (fused median <= torch median): {'met' if ok else 'NOT MET'}",
        f"noise kernel: {NOISE_BYTES} B per Gaussian = {NOISE_BYTES * N / 1e6:.1f} MB algorithmic -> {rate / 1e12:.2f} TB/s = "
        f"{100 * rate / HBM_PEAK:.1f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak ({100 * rate / HBM_COPY:.1f} % of the {HBM_COPY / 1e12:.1f} TB/s a copy achieves)",
        f"outputs after one call: max |HIP - torch| {diff:.3e} (largest move {moved:.3e})",
        f"relocate, {n_rel} dead rows ({100 * n_rel / N:.1f} %): gc_mcmc_dead + 8-byte read-back + multinomial + gc_mcmc_relocate, in place: "
        f"median {rel_med:.3f} ms, min {rel_min:.3f} ms",
        f"add_new, {n_add} new rows ({100 * n_add / N:.1f} %): weights + read-back + multinomial + 18 grown tensors + gc_mcmc_relocate: "
        f"median {add_med:.3f} ms, min {add_min:.3f} ms",
    ]
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
