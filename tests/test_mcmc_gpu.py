"""GPU tests of the MCMC densification (csrc/train_mcmc.hip, gaussctrl_amd/mcmc.py, gc_trainer.McmcCallback) against a float64 restatement
of include/gaussctrl_mcmc.h written in this file (`_sigmoid64`, `_restate_relocate`, `_restate_noise`).  The reference project has no such
strategy: the header is the contract, and these tests hold the kernels to it.

Inputs sit away from every threshold: `_guard` asserts, in float64, that every quantity a decision compares (sigmoid against min_opacity, o_new
against the clamp, o against the gate's overflow point) is at least 1e-4 relative from it; that assertion guards the inputs, not the kernel.

Tolerances (from the number formats, eps = 2^-24 = half an ulp of float32, relative):
  weights      a float32 sigmoid of a float32 logit: 2 eps relative (the issue's bound).
  new opacity  L = logit(p), p = clamp(o_new): 4 eps |L| for the logit itself (log, log1p, the difference, the final rounding: one eps each),
               plus, where the clamp does not bite, 4 eps relative on o_new (the issue's 3 eps for the expm1 form + 1 for its argument), which
               moves the logit by 4 eps / (1 - p).  Where the clamp bites p is min_opacity exactly and only the first term remains.
  new scales   s + log(o / D): eps |s_new| for the add, eps |log(o / D)| for the logarithm, 2 eps for o and the quotient, and for D, whose sum
               cancels, 2 eps * cond with cond = sum|terms| / |sum terms| of the header's double sum evaluated in float64 (one rounding
               per term and one per partial sum of a float32 evaluation; the kernel sums in double and sits far inside):
               eps * (2 cond + 2 + |log(o / D)| + |s_new|).  Constant 2, per row, nothing fitted to the kernel's output.
  noise        mean' = mean + R diag(exp(2 s)) R^T n * g * scaler: eps |mean'| for the final rounding plus K eps A g scaler, A = the sum of
               the absolute terms of the two 3 x 3 products (sum_jk |R_ik| exp(2 s_k) |R_jk| |n_j|) and K = E_g + 6: 2 eps for the float32
               expf of 2 s (one ulp), 1 for g * scaler, 3 for the products' roundings, and E_g for the float32 gate g = 1 / (1 + exp(100 (o -
               0.005))): o carries 4 eps (expf, the add, the division, + 1), the exponent's argument therefore 100 (4 o + 0.005) eps
               + 2 eps |arg|, the exponential turns that absolute error into a relative one and adds 2 eps, the add and the division one each:
               E_g = 100 (4 o + 0.005) + 2 |arg| + 4.
Everything else (dead set, order, counts, mult, untouched rows, zeroed moments, copies) is compared bit for bit."""
import ctypes as C
import math
import types

import pytest
import torch

from _margins import within
from _redzone import on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
SIZES = (1, 255, 256, 257, 70001)
SCAN_CHUNK = (65536, 65537)               # exactly 256 workgroup counts and one more: the chunk boundary of the one-workgroup scan's carry
MIN_OP = 0.005
MIN_OP32 = float(torch.tensor(MIN_OP, dtype=torch.float32))          # what the C ABI receives
MAX_OP = 1.0 - 2.0 ** -23


def _lib():
    from gaussctrl_amd import _lib as L
    return L


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _sigmoid64(logits):
    return torch.sigmoid(logits.double().reshape(-1))


def _guard(values, threshold, what):
    if values.numel():
        rel = float(((values.double() - threshold).abs() / abs(threshold)).min())
        assert rel >= 1e-4, f"a test input ({what}) sits {rel:.3g} (relative) from {threshold}: move it"


def _pick(g, n, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


# ------------------------------------------------------------------------------------------------------------ dead
def _dead(op, min_opacity=MIN_OP):
    L = _lib(); lib = L.lib()
    N = op.shape[0]
    d = on_device(op, DEV)
    weights = torch.full((N,), float("nan"), device=DEV); dead_idx = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    nb = lib.gc_mcmc_dead_workspace_bytes(L.i64(N))
    ws = torch.empty(nb // 4 + 1, dtype=torch.int32, device=DEV)
    L.check(lib.gc_mcmc_dead(L.i64(N), L.ptr(d), L.f32(min_opacity), L.ptr(weights), L.ptr(dead_idx), L.ptr(counts), L.ptr(ws), C.c_size_t(nb),
                             L.stream_ptr()), "gc_mcmc_dead")
    torch.cuda.synchronize()
    return weights.cpu(), dead_idx.cpu(), [int(v) for v in counts.cpu()], d


def _check_dead(op, tag):
    N = op.shape[0]
    a64 = _sigmoid64(op)
    _guard(a64, MIN_OP32, "sigmoid vs min_opacity")
    dead = a64 <= MIN_OP32
    weights, dead_idx, counts, d = _dead(op)
    assert _bits(d.cpu(), op)                                              # the input is not written
    n_dead = int(dead.sum())
    assert counts == [n_dead, N - n_dead]
    assert torch.equal(dead_idx[:n_dead].long(), torch.where(dead)[0])     # ascending order
    assert bool((dead_idx[n_dead:] == -1).all())                           # the rest is not written
    assert _bits(weights[dead], torch.zeros(n_dead))                       # exactly +0
    if n_dead < N:
        within(f"dead weights {tag} (x 2 eps)", ((weights[~dead].double() - a64[~dead]).abs() / (2 * EPS * a64[~dead])).max(), 1.0)
    return n_dead


@pytest.mark.parametrize("N", SIZES + SCAN_CHUNK)
def test_dead(N):
    g = torch.Generator().manual_seed(300 + N)
    alpha = _pick(g, N, [0.6, 0.3, 0.02, 0.0051, 0.0049, 0.004, 0.001])
    if N >= 16:
        alpha[0], alpha[-1], alpha[1] = 0.001, 0.004, 0.6                  # the first and the last row dead
    n_dead = _check_dead(torch.logit(alpha)[:, None].contiguous(), f"N={N}")
    assert N < 16 or 0 < n_dead < N


def test_dead_all_none_and_weights_of_all_rows():
    N = 1000
    g = torch.Generator().manual_seed(7)
    assert _check_dead(torch.logit(_pick(g, N, [0.004, 0.001, 0.0001]))[:, None].contiguous(), "all dead") == N
    op = torch.logit(_pick(g, N, [0.6, 0.3, 0.02, 0.0051]))[:, None].contiguous()
    assert _check_dead(op, "none dead") == 0
    # min_opacity = 0 (what add_new asks for): nothing is dead, the weights are the sigmoid of every row
    op = torch.logit(_pick(g, N, [0.6, 0.004, 0.001]))[:, None].contiguous()
    weights, _, counts, _ = _dead(op, 0.0)
    assert counts == [0, N]
    a64 = _sigmoid64(op)
    within("weights of all rows (x 2 eps)", ((weights.double() - a64).abs() / (2 * EPS * a64)).max(), 1.0)


# ------------------------------------------------------------------------------------------------------------ relocate
def _scene(N, seed, rest_k):
    g = torch.Generator().manual_seed(seed)
    P = {"means": torch.randn(N, 3, generator=g) * 2, "scales": torch.log(torch.rand(N, 3, generator=g) * 0.05 + 0.002),
         "quats": torch.randn(N, 4, generator=g) + 0.1, "opacities": torch.logit(_pick(g, N, [0.6, 0.3, 0.1, 0.02]))[:, None],
         "features_dc": torch.randn(N, 3, generator=g), "features_rest": torch.randn(N, rest_k, 3, generator=g) * 0.1}
    return {k: P[k].contiguous() for k in NAMES}


def _moments(P, seed):
    g = torch.Generator().manual_seed(seed)
    return ({k: torch.randn(v.shape, generator=g) * 1e-3 for k, v in P.items()}, {k: torch.rand(v.shape, generator=g) * 1e-6 for k, v in P.items()})


def _case(N, inplace, seed):
    """sampled / dest of one call: multiplicities 60 (row N - 1, o = 0.99), 7 (row 0, o = 0.3), 50 (o = 0.006: r = 51, the clamp bites), 2 (o =
    0.1), 1 (o = 0.5), fillers of multiplicity 2 and 1, every other row 0; one entry with sampled = N and one with sampled = -1 (skipped).
    Returns (sampled [n], dest [n] | None, opacity overrides {row: o})."""
    g = torch.Generator().manual_seed(seed)
    if N == 1:
        assert not inplace
        return torch.tensor([0, 0], dtype=torch.int32), None, {0: 0.3}
    others = (torch.randperm(N - 2, generator=g) + 1).tolist()            # rows 1 .. N - 2 in random order
    a, b, c = others[:3]
    key = {N - 1: (60, 0.99), 0: (7, 0.3), a: (50, 0.006), b: (2, 0.1), c: (1, 0.5)}
    n_fill = 40 if inplace and N < 1000 else 150
    fill = others[3:3 + n_fill]
    draws = [r for r, (m, _) in key.items() for _ in range(m)] + [r for k, r in enumerate(fill) for _ in range(2 - k % 2)]
    draws = [draws[i] for i in torch.randperm(len(draws), generator=g).tolist()]
    draws.insert(len(draws) // 3, N); draws.insert(2 * len(draws) // 3, -1)        # the two entries out of range
    sampled = torch.tensor(draws, dtype=torch.int32)
    dest = None
    if inplace:
        free = others[3 + n_fill:]
        assert len(free) >= len(draws)
        dest = torch.tensor(free[:len(draws)], dtype=torch.int32)                  # distinct, disjoint from the sources, in no order
    if len(draws) > 256:                                                           # duplicates of one source in different 256-blocks
        where = torch.where(sampled == N - 1)[0]
        assert int(where.min()) < 256 <= int(where.max())
    return sampled, dest, {r: o for r, (_, o) in key.items()}


def _restate_relocate(P, sampled, min_op):
    """float64: mult, and for every drawn row its new log-scale increment, new opacity logit and their bounds (module docstring)"""
    N = P["means"].shape[0]
    ok = (sampled >= 0) & (sampled < N)
    mult = torch.bincount(sampled[ok].long(), minlength=N).to(torch.int32)
    rows = torch.where(mult > 0)[0]
    out = {}
    for i in rows.tolist():
        r = min(int(mult[i]) + 1, 51)
        o = float(_sigmoid64(P["opacities"][i]))
        o_new = -math.expm1(math.log1p(-o) / r)
        terms = [math.comb(ip - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1) for ip in range(1, r + 1) for k in range(ip)]
        D = math.fsum(terms)
        cond = math.fsum(abs(t) for t in terms) / abs(D)
        inc = math.log(o / D)
        p = min(max(o_new, min_op), MAX_OP)
        clamped = o_new < min_op
        logit = math.log(p) - math.log1p(-p)
        s_new = P["scales"][i].double() + inc
        out[i] = dict(r=r, o=o, o_new=o_new, cond=cond, inc=inc, s_new=s_new, logit=logit, clamped=clamped,
                      bar_s=EPS * (2 * cond + 2 + abs(inc) + s_new.abs()), bar_op=EPS * (4 * abs(logit) + (0.0 if clamped else 4.0 / (1 - p))))
    return mult, out


def _relocate(P, mom, sampled, dest, n_rows, min_op=MIN_OP):
    """gc_mcmc_relocate on device copies of P / mom padded with NaN rows up to n_rows -> (params, exp_avg, exp_avg_sq as CPU lists, mult)"""
    L = _lib(); lib = L.lib()
    N = P["means"].shape[0]

    def dev(t):
        if t is None:
            return None
        out = torch.full((n_rows,) + tuple(t.shape[1:]), float("nan"), device=DEV)
        out[:N] = t.to(DEV)
        return out

    arr = lambda ts: (C.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in ts])
    ts = [[dev(P[k]) for k in NAMES]] + [[None if m is None else dev(m[k]) for k in NAMES] for m in mom]
    mult = torch.full((max(N, 1),), -3, dtype=torch.int32, device=DEV)
    s = on_device(sampled, DEV)
    d = None if dest is None else on_device(dest, DEV)
    rest = int(P["features_rest"][0].numel()) if N else 45
    L.check(lib.gc_mcmc_relocate(L.i64(N), L.i64(s.numel()), L.i32(rest), L.ptr(s), L.ptr(d), L.f32(min_op), L.ptr(mult), arr(ts[0]),
                                 None if mom[0] is None else arr(ts[1]), None if mom[1] is None else arr(ts[2]), L.stream_ptr()), "gc_mcmc_relocate")
    torch.cuda.synchronize()
    return [[None if t is None else t.cpu() for t in group] for group in ts], mult.cpu()[:N]


def _run_relocate(N, inplace, rest_k, moments, seed):
    P = _scene(N, seed, rest_k)
    sampled, dest, ops = _case(N, inplace, seed + 1)
    for row, o in ops.items():
        P["opacities"][row, 0] = float(torch.logit(torch.tensor(o, dtype=torch.float64)))
    n = sampled.numel()
    n_rows = N if inplace else N + n
    mom = _moments(P, seed + 2) if moments == "all" else (None, None)
    if moments == "some":
        mom = _moments(P, seed + 2)
        for k in ("means", "features_rest"):
            mom[0][k] = None; mom[1][k] = None
    mult64, ref = _restate_relocate(P, sampled, MIN_OP32)
    _guard(torch.tensor([v["o_new"] for v in ref.values()]), MIN_OP32, "o_new vs the clamp")
    if N > 1:
        assert sorted(set(mult64.tolist())) == [0, 1, 2, 7, 50, 60]
        assert ref[N - 1]["r"] == 51 and ref[0]["r"] == 8 and sum(v["clamped"] for v in ref.values()) == 1
        assert max(v["cond"] for v in ref.values()) > 10                   # the cancellation the bound is about is in the test
    (got, gm, gv), mult = _relocate(P, mom, sampled, dest, n_rows)
    assert torch.equal(mult, mult64)
    ok = (sampled >= 0) & (sampled < N)
    dst = (dest if inplace else torch.arange(N, N + n, dtype=torch.int32)).long()
    src_rows = torch.where(mult64 > 0)[0]
    touched = torch.zeros(n_rows, dtype=torch.bool)
    touched[src_rows] = True; touched[dst[ok]] = True
    pad = lambda t: torch.cat([t, torch.full((n_rows - N,) + tuple(t.shape[1:]), float("nan"))], 0)
    worst_s = worst_op = 0.0
    for t, name in enumerate(NAMES):
        before = pad(P[name])
        assert _bits(got[t][~touched], before[~touched]), name                         # untouched rows (the skipped entries' rows among them)
        if name not in ("scales", "opacities"):
            assert _bits(got[t][src_rows], before[src_rows]), name                     # a source keeps everything but scales and opacity
        assert _bits(got[t][dst[ok]], got[t][sampled[ok].long()]), name                # a copy is its UPDATED source, bit for bit
        for j, gmom in ((0, gm), (1, gv)):
            if mom[j] is None or mom[j][name] is None:
                assert gmom[t] is None
                continue
            mb = pad(mom[j][name])
            assert _bits(gmom[t][~touched], mb[~touched]), (name, j)
            assert _bits(gmom[t][touched], torch.zeros_like(gmom[t][touched])), (name, j)          # exactly +0
    for i, v in ref.items():
        worst_s = max(worst_s, float(((got[1][i].double() - v["s_new"]).abs() / v["bar_s"]).max()))
        worst_op = max(worst_op, abs(float(got[3][i, 0]) - v["logit"]) / v["bar_op"])
    return worst_s, worst_op


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("inplace", [True, False])
def test_relocate(N, inplace):
    if N == 1 and inplace:
        # one row cannot be source and destination: n = 0 on it, nothing moves
        P = _scene(1, 5, 15)
        mom = _moments(P, 6)
        (got, gm, gv), _ = _relocate(P, mom, torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 1)
        for t, k in enumerate(NAMES):
            assert _bits(got[t], P[k]) and _bits(gm[t], mom[0][k]) and _bits(gv[t], mom[1][k])
        return
    ws, wo = _run_relocate(N, inplace, 15, "all", seed=400 + N)
    within(f"relocate scales N={N} inplace={inplace} (x bar)", ws, 1.0)
    within(f"relocate opacities N={N} inplace={inplace} (x bar)", wo, 1.0)


@pytest.mark.parametrize("rest_k,moments", [(0, "all"), (3, "some"), (15, "none"), (3, "none"), (15, "some")])
def test_relocate_sh_widths_and_missing_moments(rest_k, moments):
    for inplace in (True, False):
        ws, wo = _run_relocate(1500, inplace, rest_k, moments, seed=500 + rest_k)
        within(f"relocate scales R={3 * rest_k} {moments} (x bar)", ws, 1.0)
        within(f"relocate opacities R={3 * rest_k} {moments} (x bar)", wo, 1.0)


def test_relocate_nothing_to_do():
    """n = 0: success, nothing written (mult included)"""
    P = _scene(300, 9, 15)
    mom = _moments(P, 10)
    (got, gm, gv), mult = _relocate(P, mom, torch.zeros(0, dtype=torch.int32), None, 300)
    for t, k in enumerate(NAMES):
        assert _bits(got[t], P[k]) and _bits(gm[t], mom[0][k]) and _bits(gv[t], mom[1][k])
    assert bool((mult == -3).all())


def test_restatement_identities():
    """r = 1 (cannot occur in a call): the restated formulas give o_new = o and D = o; and the single sum the kernel evaluates is the header's
    double sum"""
    for o in (0.006, 0.3, 0.99):
        assert abs(-math.expm1(math.log1p(-o)) - o) <= 1e-14 * o
    for r, o_new in ((1, 0.3), (8, 0.04), (51, 0.0863), (51, 1.2e-4)):
        double = math.fsum(math.comb(ip - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1) for ip in range(1, r + 1) for k in range(ip))
        single = math.fsum(math.comb(r, m) * (-1.0) ** (m - 1) * o_new ** m / math.sqrt(m) for m in range(1, r + 1))
        assert abs(double - single) <= 1e-9 * abs(double)
        if r == 1:
            assert double == o_new


# ------------------------------------------------------------------------------------------------------------ noise
def _restate_noise(P, noise, scaler):
    q = P["quats"].double()
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    e = torch.exp(2 * P["scales"].double())
    cov = R @ torch.diag_embed(e) @ R.transpose(1, 2)
    o = _sigmoid64(P["opacities"])
    arg = 100 * (o - 0.005)
    g = 1 / (1 + torch.exp(arg))
    want = P["means"].double() + (cov @ noise.double()[..., None])[..., 0] * (g * scaler)[:, None]
    A = ((R.abs() * e[:, None, :]) @ (R.abs().transpose(1, 2) @ noise.double().abs()[..., None]))[..., 0]
    K = 100 * (4 * o + 0.005) + 2 * arg.abs() + 4 + 6
    bar = EPS * want.abs() + EPS * K[:, None] * A * (g * scaler)[:, None]
    return want, bar, o


def _noise_call(P, noise, scaler):
    L = _lib(); lib = L.lib()
    N = P["means"].shape[0]
    d = {k: on_device(P[k], DEV) for k in ("means", "scales", "quats", "opacities")}
    nz = on_device(noise, DEV)
    L.check(lib.gc_mcmc_inject_noise(L.i64(N), L.ptr(d["means"]), L.ptr(d["scales"]), L.ptr(d["quats"]), L.ptr(d["opacities"]), L.ptr(nz),
                                     L.f32(scaler), L.stream_ptr()), "gc_mcmc_inject_noise")
    torch.cuda.synchronize()
    for k in ("scales", "quats", "opacities"):
        assert _bits(d[k].cpu(), P[k]), k                                  # never written
    assert _bits(nz.cpu(), noise)
    return d["means"].cpu()


@pytest.mark.parametrize("N", SIZES)
def test_inject_noise(N):
    g = torch.Generator().manual_seed(600 + N)
    P = _scene(N, 601 + N, 0)
    P["quats"] = (torch.randn(N, 4, generator=g) * 2 + 0.3).contiguous()                # unnormalised
    P["scales"] = torch.log(torch.rand(N, 3, generator=g) * 0.5 + 0.004).contiguous()   # anisotropic, 0.004 .. 0.5
    alpha = _pick(g, N, [0.001, 0.004, 0.02, 0.95])
    if N >= 16:
        alpha[:4] = torch.tensor([0.001, 0.004, 0.02, 0.95]); alpha[-1] = 0.95
    P["opacities"] = torch.logit(alpha)[:, None].contiguous()
    noise = torch.randn(N, 3, generator=g)
    scaler = 80.0                                                          # lr 1.6e-4 x noise_lr 5e5
    want, bar, o = _restate_noise(P, noise, scaler)
    _guard(o, 0.885, "o vs the overflow point of the gate")
    got = _noise_call(P, noise, scaler)
    gated = o > 0.885
    assert _bits(got[gated], P["means"][gated])                            # g = 0 exactly: the means keep their bits
    live = ~gated
    if live.any():
        assert not _bits(got[live], P["means"][live])                      # the others moved
        within(f"inject_noise N={N} (x bar)", ((got[live].double() - want[live]).abs() / bar[live]).max(), 1.0)
    assert _bits(_noise_call(P, noise, 0.0), P["means"])                   # scaler = 0: bit-identical


# ------------------------------------------------------------------------------------------------------------ host layer
def _model(N, seed=31, dead_frac=0.1, **cfg):
    """a stand-alone model with stepped Adam state (two optimizer steps on random gradients: no render needed)"""
    from gaussctrl_amd.gc_config import build_optimizers
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    g = torch.Generator().manual_seed(seed)
    P = _scene(N, seed, 15)
    alpha = _pick(g, N, [0.6, 0.3, 0.1, 0.02])
    alpha[torch.rand(N, generator=g) < dead_frac] = 0.002
    P["opacities"] = torch.logit(alpha)[:, None].contiguous()
    model = GaussCtrlModel(GaussCtrlModelConfig(densify_strategy="mcmc", **cfg), params=P, device=DEV)
    opts = build_optimizers(model)
    for _ in range(2):
        for o in opts.values():
            for p in o.param_groups[0]["params"]:
                p.grad = torch.randn(p.shape, generator=g).to(DEV) * 1e-3
            o.step()
    for o in opts.values():
        o.zero_grad(set_to_none=True)
    return model, opts


def _state_of(model, opts):
    from gaussctrl_amd.scene_rows import owners
    return {n: (opt, p, opt.state[p]) for n, (opt, p) in owners(model, opts).items()}


def test_host_relocate():
    from gaussctrl_amd import mcmc
    from gaussctrl_amd._lib import GaussCtrlHipError
    N = 3000
    model, opts = _model(N)
    with torch.no_grad():                                                  # keep the dead rows dead and guarded after the two Adam steps
        a = torch.sigmoid(model.opacities.data)
        model.opacities.data[a < 0.01] = float(torch.logit(torch.tensor(0.002)))
    before = {n: getattr(model, n).detach().cpu().clone() for n in NAMES}
    a64 = _sigmoid64(before["opacities"])
    _guard(a64, MIN_OP32, "sigmoid vs min_opacity")
    dead = a64 <= MIN_OP32
    n_dead = int(dead.sum())
    assert 100 < n_dead < N // 2
    st = _state_of(model, opts)
    ptrs = {n: (p.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr(), s["step"]) for n, (_, p, s) in st.items()}
    # a caller's draws are validated
    live = torch.where(~dead)[0]
    with pytest.raises(ValueError):
        mcmc.relocate(model, opts, live[:n_dead - 1].to(DEV))
    with pytest.raises(ValueError):
        mcmc.relocate(model, opts, torch.full((n_dead,), N, device=DEV))
    with pytest.raises(ValueError):
        mcmc.relocate(model, opts, torch.where(dead)[0].to(DEV))
    with pytest.raises(ValueError):
        mcmc.relocate(model, opts, live[:n_dead].float().to(DEV))
    with pytest.raises(GaussCtrlHipError):
        mcmc.relocate(model, opts, live[:n_dead])
    assert all(_bits(getattr(model, n).detach().cpu(), before[n]) for n in NAMES)          # a refused call changed nothing
    model.means.grad = torch.zeros_like(model.means)
    torch.manual_seed(3)
    assert mcmc.relocate(model, opts) == n_dead
    assert model.num_points == N and model.means.grad is None
    st = _state_of(model, opts)
    assert ptrs == {n: (p.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr(), s["step"]) for n, (_, p, s) in st.items()}
    after = {n: getattr(model, n).detach().cpu() for n in NAMES}
    # no dead row remains, except a copy whose opacity the clamp set to min_opacity itself
    left = _sigmoid64(after["opacities"]) <= MIN_OP32
    lim = math.log(MIN_OP32) - math.log1p(-MIN_OP32)
    assert bool(((after["opacities"].double().reshape(-1)[left] - lim).abs() <= 4 * EPS * abs(lim)).all())
    # default sampling never picks a dead row: every formerly dead row is now a copy (means included) of a row that was alive
    alive_means = {tuple(r) for r in before["means"][~dead].tolist()}
    dead_means = {tuple(r) for r in before["means"][dead].tolist()}
    assert alive_means.isdisjoint(dead_means)
    assert all(tuple(r) in alive_means for r in after["means"][dead].tolist())
    assert _bits(after["means"][~dead], before["means"][~dead])
    # the copies and their sources have zero moments; rows that were neither keep theirs
    copied = {tuple(r) for r in after["means"][dead].tolist()}
    src = torch.tensor([tuple(r) in copied for r in after["means"].tolist()])
    m = st["scales"][2]["exp_avg"].cpu()
    assert bool((m[src] == 0).all()) and bool((m[~src].abs().amax(-1) > 0).all())
    assert 0 <= mcmc.relocate(model, opts) <= n_dead                       # (a second call finds at most the clamped copies)


def test_host_add_new():
    from gaussctrl_amd import mcmc
    N = 1000
    model, opts = _model(N)
    before = {n: getattr(model, n).detach().cpu().clone() for n in NAMES}
    steps = {n: s["step"] for n, (_, _, s) in _state_of(model, opts).items()}
    model.config.mcmc_cap_max = 10_000
    assert mcmc.add_new(model, opts) == 50 and model.num_points == 1050                    # int(1.05 * 1000)
    model.config.mcmc_cap_max = 1060
    assert mcmc.add_new(model, opts) == 10 and model.num_points == 1060                    # the cap, not int(1.05 * 1050) = 1102
    assert mcmc.add_new(model, opts) == 0 and model.num_points == 1060                     # at the cap: nothing
    model.config.mcmc_cap_max = 500
    assert mcmc.add_new(model, opts) == 0 and model.num_points == 1060                     # over the cap: nothing either
    st = _state_of(model, opts)
    for n, (opt, p, s) in st.items():
        assert len(opt.state) == 1 and p.shape[0] == 1060 and p.grad is None
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape and s["step"] == steps[n]
        assert float(s["exp_avg"][N:].abs().max()) == 0.0 and float(s["exp_avg_sq"][N:].abs().max()) == 0.0      # new rows: zero moments
        if n not in ("scales", "opacities"):
            assert _bits(p.detach().cpu()[:N], before[n])
    # every new row is a copy of one of the first 1050 rows (sources of the second call may be rows the first call added)
    old = {tuple(r) for r in model.means.detach().cpu()[:1050].tolist()}
    assert all(tuple(r) in old for r in model.means.detach().cpu()[N:].tolist())
    # a caller's draws
    model.config.mcmc_cap_max = 1062
    with pytest.raises(ValueError):
        mcmc.add_new(model, opts, torch.tensor([5, 1060], device=DEV))
    assert mcmc.add_new(model, opts, torch.tensor([5, 5], device=DEV)) == 2
    got = model.means.detach().cpu()
    assert _bits(got[1060], got[5]) and _bits(got[1061], got[5])
    o5 = model.opacities.detach().cpu()
    assert _bits(o5[1060], o5[5]) and _bits(o5[1061], o5[5])


def test_host_inject_noise_validates():
    from gaussctrl_amd import mcmc
    from gaussctrl_amd._lib import GaussCtrlHipError
    model, _ = _model(300)
    before = model.means.detach().clone()
    with pytest.raises(ValueError):
        mcmc.inject_noise(model, 1e-4, torch.zeros(299, 3, device=DEV))
    with pytest.raises(ValueError):
        mcmc.inject_noise(model, 1e-4, torch.zeros(300, 3, device=DEV, dtype=torch.float64))
    with pytest.raises(GaussCtrlHipError):
        mcmc.inject_noise(model, 1e-4, torch.zeros(300, 3))
    assert torch.equal(model.means.detach(), before)
    noise = torch.randn(300, 3, device=DEV)
    mcmc.inject_noise(model, 1e-4, noise)
    P = {k: getattr(model, k).detach().cpu() for k in ("scales", "quats", "opacities")}
    P["means"] = before.cpu()
    want, bar, _ = _restate_noise(P, noise.cpu(), float(torch.tensor(1e-4 * 5e5, dtype=torch.float32)))
    assert bool(((model.means.detach().cpu().double() - want).abs() <= bar).all()) and not torch.equal(model.means.detach(), before)


def test_mcmc_callback_run():
    """~35 steps of the built-in iteration order on a 2000-Gaussian scene at 64 x 64: refinement at steps 5, 10, 15, 20, 25 (start 4, stop 30,
    every 5), the cap two and a half growth steps away"""
    from gaussctrl_amd import mcmc, synthetic as syn
    from gaussctrl_amd.gc_config import build_optimizers
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.gc_trainer import McmcCallback, StepCallback, TrainingCallbackAttributes
    from gaussctrl_amd.ns_compat import Cameras
    P = syn.make_gaussians(2000, seed=21, scale_mean=0.05)
    P["opacities"][:20] = math.log(0.001 / 0.999)                          # dead at the first refinement step whatever five Adam steps do
    cams = Cameras(syn.make_cameras(4, seed=22), 60.0, 60.0, 32.0, 32.0, 64, 64)
    cap = 2300
    cfg = GaussCtrlModelConfig(background_color="black", densify_strategy="mcmc", refine_on_device=True, mcmc_refine_every=5, mcmc_refine_start_iter=4,
                               mcmc_refine_stop_iter=30, mcmc_cap_max=cap, sh_degree_interval=1)
    model = GaussCtrlModel(cfg, params=P, device=DEV)
    model.train()
    target_model = GaussCtrlModel(GaussCtrlModelConfig(background_color="black", sh_degree_interval=1), params={k: v.copy() for k, v in P.items()}, device=DEV)
    with torch.no_grad():
        target_model.features_dc += 0.3
        targets = [target_model.get_outputs_for_camera(cams[i])["rgb"].clone() for i in range(4)]
    opts = build_optimizers(model)
    cbs = model.get_training_callbacks(TrainingCallbackAttributes(optimizers=opts, grad_scaler=None, pipeline=None))
    assert [type(c) for c in cbs] == [StepCallback, McmcCallback]
    step_cb, mcb = cbs
    sizes = [model.num_points]

    def iteration(step):
        """zero_grad / forward / loss / backward / optimizer step in a scope of its own, as the trainer's train_iteration: no loss graph of
        this step outlives it (a held graph keeps the gradient accumulators of the old row count alive across a growth step)"""
        for o in opts.values():
            o.zero_grad(set_to_none=True)
        loss_dict = model.get_loss_dict(model.get_outputs(cams[step % 4]), {"image": targets[step % 4]})
        assert sorted(loss_dict) == ["main_loss", "opacity_reg", "scale_reg"]
        loss = sum(loss_dict.values())
        loss.backward()
        for o in opts.values():
            o.step()
        return float(loss.detach())

    for step in range(35):
        step_cb.run_callback_at_location(step, "before_train_iteration")
        assert math.isfinite(iteration(step))
        snap = {n: getattr(model, n).detach().clone() for n in ("means", "scales", "quats")}
        n_before = model.num_points
        refine = mcmc.schedule(cfg, step)
        assert refine == (step in (5, 10, 15, 20, 25))
        torch.manual_seed(step)
        mcb.run_callback_at_location(step, "after_train_iteration")
        want = min(cap, int(1.05 * n_before)) if refine else n_before
        assert model.num_points == max(want, n_before), (step, model.num_points, want)
        sizes.append(model.num_points)
        assert not torch.equal(model.means.detach()[:n_before], snap["means"])              # the noise moved means at every step
        if not refine:                                                                      # scales and quats change only through Adam
            assert torch.equal(model.scales.detach(), snap["scales"]) and torch.equal(model.quats.detach(), snap["quats"])
        for n in NAMES:
            assert bool(torch.isfinite(getattr(model, n).detach()).all()), (step, n)
        for o in opts.values():
            for p in o.param_groups[0]["params"]:
                assert p.shape[0] == model.num_points and o.state[p]["exp_avg"].shape == p.shape
    assert sorted(set(sizes)) == [2000, 2100, 2205, 2300] and sizes[-1] == cap
    assert mcb.n_added == cap - 2000 and mcb.n_relocated >= 20
    model.eval()
    with torch.no_grad():
        assert bool(torch.isfinite(model.get_outputs(cams[0])["rgb"]).all())


def test_mcmc_refuses_more_than_one_gpu():
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline
    me = types.SimpleNamespace(world_size=2, model=types.SimpleNamespace(config=GaussCtrlModelConfig(densify_strategy="mcmc")),
                               config=types.SimpleNamespace(train_mode="throughput"))
    with pytest.raises(ValueError, match="mcmc"):
        GaussCtrlPipeline.train_forward_backward(me, 0)
