"""GPU tests of the device refinement (csrc/train_refine.hip, gaussctrl_amd/refine.py, gc_trainer.RefineCallback) against a float64 torch
restatement of nerfstudio 1.0.0's after_train / refinement_after written in this file (`_restate`, `_restate_accumulate`).

Inputs sit away from every threshold: `_guard` asserts, in float64, that every quantity a decision compares is at least 1e-4 relative from
its threshold, so that no float32 / float64 knife edge decides an action (that assertion guards the inputs, not the kernel).

Tolerances (all from the number formats, eps = 2^-24):
  accumulate   grad_norm_sum: per accumulated term one sqrt (0.5 ulp; the sum of squares under it adds 1 ulp to its argument = 0.5 ulp of the
               root) and one add: <= 4 eps * sum of the terms.  max_2dsize: 1 / max(H, W) rounded once, one product: 2 eps relative.
  child scales s - log 1.6: the constant rounded once (eps * 0.47), one subtraction: 4 eps relative + 2^-23 absolute (the issue's bound).
  child means  16 eps * (|mean|_inf + |exp(scale) * z|_inf) (the issue's bound).
Everything else (action words, counts, row placement, copied values, moments) is compared bit for bit."""
import math

import pytest
import torch

from _margins import within
from _redzone import on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
KEEP, SPLIT, DUP, EMIT_SPLIT, EMIT_DUP, BELOW_ALPHA, TOO_BIG, ON_SCREEN = 1, 2, 4, 8, 16, 32, 64, 128
NAMES = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")
SIZES = (1, 255, 256, 257, 70001)
SCAN_CHUNK = (65536, 65537)               # exactly 256 workgroup counts and one more: the chunk boundary of the one-workgroup scan's carry

# thresholds of the populations below (splatfacto's defaults except where a smaller scene needs another scale)
TH = dict(max_dim=64.0, densify_grad_thresh=0.0002, densify_size_thresh=0.01, split_screen_size=0.05, cull_alpha_thresh=0.1,
          cull_scale_thresh=0.5, cull_screen_size=0.15)


def _lib():
    from gaussctrl_amd import _lib as L
    return L


# ------------------------------------------------------------------------------------------------------------ the restatement (float64)
def _restate_accumulate(stats, xys_grad, radii, max_dim):
    """stats: 3 float64 [N] tensors (CPU), updated for ONE view as splatfacto's after_train does"""
    s, c, m = stats
    vis = radii > 0
    g = xys_grad.double()
    s[vis] += torch.sqrt(g[vis, 0] ** 2 + g[vis, 1] ** 2)
    c[vis] += 1
    m[vis] = torch.maximum(m[vis], radii[vis].double() / max_dim)


def _restate(P, stats, th, densify, ns, split_by_screen, cull_by_scale, cull_by_screen):
    """Section 2 of the refinement specification in float64 on CPU tensors.  P: the six float32 tensors; stats: (grad_norm_sum, vis_count,
    max_2dsize) as the device holds them (float32) or None.  Returns a dict with the action word, the counts, for every output row its
    source (`src`), kind (0 survivor, 1 split child, 2 duplicate) and split sample index, and the guard margins."""
    N = P["means"].shape[0]
    sc = P["scales"].double()
    smax = sc.exp().max(dim=-1).values if N else torch.zeros(0, dtype=torch.float64)
    alpha = torch.sigmoid(P["opacities"].double().reshape(-1))
    margins = []

    def cmp(v, thr, on=None):
        rel = ((v - thr).abs() / abs(thr))
        if on is not None:
            rel = rel[on]
        if rel.numel():
            margins.append(float(rel.min()))
        return v > thr

    below = ~cmp(alpha, th["cull_alpha_thresh"])
    split = torch.zeros(N, dtype=torch.bool); dup = torch.zeros(N, dtype=torch.bool)
    m2d = stats[2].double() if stats is not None else torch.zeros(N, dtype=torch.float64)
    if densify:
        gs, cnt = stats[0].double(), stats[1].double()
        seen = cnt > 0
        avg = torch.where(seen, gs / cnt.clamp(min=1) * 0.5 * th["max_dim"], torch.zeros_like(gs))
        high = cmp(avg, th["densify_grad_thresh"], seen) & seen            # never seen: NaN in torch, compares false
        big = cmp(smax, th["densify_size_thresh"])
        scr = cmp(m2d, th["split_screen_size"]) if split_by_screen else torch.zeros(N, dtype=torch.bool)
        split = (big | scr) & high
        dup = ~big & high
    too_big = cmp(smax, th["cull_scale_thresh"]) if cull_by_scale else torch.zeros(N, dtype=torch.bool)
    on_screen = cmp(m2d, th["cull_screen_size"]) if cull_by_screen else torch.zeros(N, dtype=torch.bool)
    child_big = cmp((sc - math.log(1.6)).exp().max(dim=-1).values if N else smax, th["cull_scale_thresh"], split) if cull_by_scale else too_big
    keep = ~split & ~below & ~too_big & ~on_screen
    emit_split = split & ~below & ~child_big
    emit_dup = dup & ~below & ~too_big
    action = (keep * KEEP + split * SPLIT + dup * DUP + emit_split * EMIT_SPLIT + emit_dup * EMIT_DUP + below * BELOW_ALPHA + too_big * TOO_BIG
              + on_screen * ON_SCREEN).to(torch.int32)
    surv, ssrc, dsrc = torch.where(keep)[0], torch.where(emit_split)[0], torch.where(emit_dup)[0]
    src = torch.cat([surv] + [ssrc] * ns + [dsrc])
    kind = torch.cat([torch.zeros_like(surv)] + [torch.ones_like(ssrc)] * ns + [2 * torch.ones_like(dsrc)])
    counts = [len(surv), len(ssrc), len(dsrc), len(src), int((below * (1 + split * ns + dup * 1)).sum())]
    ranks = torch.stack([torch.cumsum(f.int(), 0) - f.int() for f in (keep, emit_split, emit_dup)]).to(torch.int32) if N else torch.zeros(3, 0, dtype=torch.int32)
    return dict(action=action, counts=counts, src=src, kind=kind, ranks=ranks, margin=min(margins) if margins else 1.0,
                n_surv=len(surv), n_split_src=len(ssrc))


def _guard(ref):
    assert ref["margin"] >= 1e-4, f"a test input sits {ref['margin']:.3g} (relative) from a threshold: move it"


def _child_means64(P, src, samples):
    q = P["quats"][src].double()
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    v = P["scales"][src].double().exp() * samples.double()
    return P["means"][src].double() + torch.bmm(R, v[..., None])[..., 0], v


# ------------------------------------------------------------------------------------------------------------ populations
def _pick(g, n, values):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), (n,), generator=g)]


def _population(N, seed, kind="mixed", rest_k=15):
    """Six parameter tensors + statistics (CPU float32) whose decision quantities are drawn from small sets of values far from the thresholds.
    kind: mixed (every action occurs once N is large enough; the first 16 rows enumerate them), quiet (nothing to do), dead (everything
    culled), unseen (no visible Gaussian)."""
    g = torch.Generator().manual_seed(seed)
    P = {"means": torch.randn(N, 3, generator=g) * 2, "quats": torch.randn(N, 4, generator=g) + 0.1,
         "features_dc": torch.randn(N, 3, generator=g), "features_rest": torch.randn(N, rest_k, 3, generator=g) * 0.1}
    # max scale: 0.004 (small), 0.03 (big for densify), 0.7 (over the cull scale; its children 0.4375 are not), 1.2 (children 0.75 over it too)
    smax = _pick(g, N, [0.004, 0.004, 0.004, 0.03, 0.03, 0.7, 1.2])
    alpha = _pick(g, N, [0.6, 0.6, 0.6, 0.3, 0.04])                       # 0.04 < 0.1 = cull_alpha_thresh
    cnt = _pick(g, N, [0.0, 1.0, 3.0, 3.0])
    avg = _pick(g, N, [0.00005, 0.00005, 0.0006, 0.002])                  # densify_grad_thresh 0.0002
    m2d = _pick(g, N, [0.0, 0.01, 0.01, 0.08, 0.3])                       # split_screen_size 0.05, cull_screen_size 0.15
    if kind == "mixed" and N >= 16:
        # survivor | split (big) | dup | alpha cull | scale cull | screen cull | split with children over the scale | dup below alpha |
        # split by screen size of a small one (split AND dup) | never seen but would be high | split of one over the cull scale (children fit)
        rows = [(0.004, 0.6, 3, 0.00005, 0.01), (0.03, 0.6, 3, 0.002, 0.01), (0.004, 0.6, 3, 0.002, 0.01), (0.004, 0.04, 3, 0.00005, 0.01),
                (0.7, 0.6, 3, 0.00005, 0.01), (0.004, 0.6, 3, 0.00005, 0.3), (1.2, 0.6, 3, 0.002, 0.01), (0.004, 0.04, 3, 0.002, 0.01),
                (0.004, 0.6, 3, 0.002, 0.08), (0.03, 0.6, 0, 0.002, 0.01), (0.7, 0.6, 1, 0.0006, 0.0), (0.03, 0.04, 3, 0.002, 0.0)]
        for r, (a, b, c, d, e) in enumerate(rows):
            smax[r], alpha[r], cnt[r], avg[r], m2d[r] = a, b, c, d, e
    if kind == "quiet":
        smax[:] = 0.004; alpha[:] = 0.6; avg[:] = 0.00005; m2d[:] = 0.01
    if kind == "dead":
        alpha[:] = 0.04
    if kind == "unseen":
        cnt[:] = 0.0
    ratio = torch.rand(N, 2, generator=g) * 0.8 + 0.1                      # the two smaller axes: 0.1 .. 0.9 of the largest
    sc = torch.stack([smax, smax * ratio[:, 0], smax * ratio[:, 1]], -1)
    perm = torch.argsort(torch.rand(N, 3, generator=g), dim=-1)
    P["scales"] = torch.log(torch.gather(sc, 1, perm))
    P["opacities"] = torch.logit(alpha)[:, None]
    gsum = (avg.double() * cnt.double() / (0.5 * TH["max_dim"])).float()
    if kind == "mixed" and N >= 16:
        gsum[9] = 1.0                      # never seen (count 0) with a sum that would be high: still not high
    if kind == "unseen":
        gsum[:] = 1.0
    stats = (gsum, cnt.clone(), torch.where(cnt > 0, m2d, torch.zeros_like(m2d)))
    P = {k: P[k].contiguous() for k in NAMES}
    return P, stats


def _moments(P, seed):
    g = torch.Generator().manual_seed(seed)
    return ({k: torch.randn(v.shape, generator=g) * 1e-3 for k, v in P.items()}, {k: torch.rand(v.shape, generator=g) * 1e-6 for k, v in P.items()})


# ------------------------------------------------------------------------------------------------------------ driving the C ABI
def _plan(P, stats, densify, ns, split_by_screen, cull_by_scale, cull_by_screen, th=TH):
    import ctypes as C
    L = _lib(); lib = L.lib()
    N = P["means"].shape[0]
    d = lambda t: None if t is None else on_device(t, DEV)
    sc, op = d(P["scales"]), d(P["opacities"])
    st = [d(t) for t in stats] if stats is not None else [None] * 3
    action = torch.full((N,), -1, dtype=torch.int32, device=DEV); ranks = torch.full((3, N), -1, dtype=torch.int32, device=DEV)
    counts = torch.full((5,), -1, dtype=torch.int32, device=DEV)
    nb = lib.gc_refine_plan_workspace_bytes(L.i64(N))
    ws = torch.empty(nb // 4 + 1, dtype=torch.int32, device=DEV)
    rc = lib.gc_refine_plan(L.i64(N), L.ptr(sc), L.ptr(op), L.ptr(st[0]), L.ptr(st[1]), L.ptr(st[2]), L.i32(densify), L.i32(ns),
                            L.f32(th["max_dim"]), L.f32(th["densify_grad_thresh"]), L.f32(th["densify_size_thresh"]), L.i32(split_by_screen),
                            L.f32(th["split_screen_size"]), L.f32(th["cull_alpha_thresh"]), L.i32(cull_by_scale), L.f32(th["cull_scale_thresh"]),
                            L.i32(cull_by_screen), L.f32(th["cull_screen_size"]), L.ptr(action), L.ptr(ranks), L.ptr(counts), L.ptr(ws),
                            C.c_size_t(nb), L.stream_ptr())
    return rc, action, ranks, counts


def _apply(P, mom, action, ranks, counts, ns, samples):
    import ctypes as C
    L = _lib(); lib = L.lib()
    N = P["means"].shape[0]
    n_out = counts[3]
    arr = lambda ts: (C.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in ts])
    ins = [[on_device(P[k], DEV) for k in NAMES]] + [[None if m is None or m[k] is None else on_device(m[k], DEV) for k in NAMES] for m in mom]
    outs = [[None if t is None else torch.full((n_out,) + tuple(t.shape[1:]), float("nan"), device=DEV) for t in ts] for ts in ins]
    smp = None if samples is None else on_device(samples, DEV)
    rest = int(P["features_rest"][0].numel()) if N else 45
    L.check(lib.gc_refine_apply(L.i64(N), L.i32(ns), L.i32(rest), L.i64(counts[0]), L.i64(counts[1]), L.i64(counts[2]), L.ptr(action), L.ptr(ranks),
                                L.ptr(smp), arr(ins[0]), arr(ins[1]), arr(ins[2]), arr(outs[0]), arr(outs[1]), arr(outs[2]), L.stream_ptr()),
            "gc_refine_apply")
    torch.cuda.synchronize()
    return [[None if t is None else t.cpu() for t in ts] for ts in outs]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_scene(P, mom, ref, outs, ns, samples):
    """every output tensor against the restatement's row table"""
    src, kind = ref["src"], ref["kind"]
    surv, child, spl = kind == 0, kind > 0, kind == 1
    worst_mean = worst_scale = 0.0
    for t, name in enumerate(NAMES):
        got = outs[0][t]
        assert got.shape[0] == len(src)
        want = P[name][src]
        if name == "means" and spl.any():
            m64, v = _child_means64(P, src[spl], samples)
            bar = 16 * EPS * (P["means"][src[spl]].double().abs().amax(-1) + v.abs().amax(-1))
            worst_mean = float(((got[spl].double() - m64).abs().amax(-1) / bar).max())
            assert _bits(got[~spl], want[~spl])
        elif name == "scales" and spl.any():
            s64 = P["scales"][src[spl]].double() - math.log(1.6)
            worst_scale = float(((got[spl].double() - s64).abs() / (4 * EPS * s64.abs() + 2.0 ** -23)).max())
            assert _bits(got[~spl], want[~spl])
        else:
            assert _bits(got, want), name
        for j in (0, 1):
            if mom[j] is None or mom[j][name] is None:
                assert outs[1 + j][t] is None
                continue
            gm = outs[1 + j][t]
            assert _bits(gm[surv], mom[j][name][src[surv]]), (name, j)
            assert _bits(gm[child], torch.zeros_like(gm[child])), (name, j)          # exactly +0
    return worst_mean, worst_scale


def _run_plan_apply(P, stats, mom, ns, densify=True, split_by_screen=True, cull_by_scale=True, cull_by_screen=True, seed=5):
    ref = _restate(P, stats, TH, densify, ns, split_by_screen, cull_by_scale, cull_by_screen)
    _guard(ref)
    rc, action, ranks, counts = _plan(P, stats, densify, ns, split_by_screen, cull_by_scale, cull_by_screen)
    assert rc == 0
    counts = [int(v) for v in counts.cpu()]
    assert counts == ref["counts"]
    assert torch.equal(action.cpu(), ref["action"])
    assert torch.equal(ranks.cpu(), ref["ranks"])
    samples = torch.randn(ns * counts[1], 3, generator=torch.Generator().manual_seed(seed))
    outs = _apply(P, mom, action, ranks, counts, ns, samples)
    wm, wsc = _check_scene(P, mom, ref, outs, ns, samples)
    return ref, outs, wm, wsc


# ------------------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("C", [1, 3])
def test_accumulate(N, C):
    L = _lib(); lib = L.lib()
    g = torch.Generator().manual_seed(100 + N + C)
    H, W = 48, 60
    xg = torch.randn(C, N, 2, generator=g) * torch.exp(torch.randn(C, N, 1, generator=g) * 3 - 8)
    radii = torch.randint(0, 40, (C, N), generator=g, dtype=torch.int32)
    hidden = torch.rand(N, generator=g) < 0.3
    if N > 1:
        hidden[0] = True; hidden[-1] = False
    radii[:, hidden] = 0                                                  # invisible in every view: statistics untouched
    radii[:, ~hidden] = radii[:, ~hidden].clamp(min=1) * (torch.rand(C, int((~hidden).sum()), generator=g) < 0.7).int()
    start = [torch.rand(N, generator=g) * 1e-3, torch.randint(0, 5, (N,), generator=g).float(), torch.rand(N, generator=g) * 0.2]

    def run(views):
        st = [on_device(t, DEV) for t in start]
        for v in views:
            x = on_device(xg[v], DEV); r = on_device(radii[v], DEV)
            Cv = x.shape[0]
            L.check(lib.gc_refine_accumulate_views(L.i64(N), L.i32(Cv), L.ptr(x), L.ptr(r), L.f32(1.0 / max(H, W)), L.ptr(st[0]), L.ptr(st[1]),
                                                   L.ptr(st[2]), L.stream_ptr()), "gc_refine_accumulate_views")
        return [t.cpu() for t in st]

    got = run([slice(0, C)])
    if C > 1:
        one = run([slice(v, v + 1) for v in range(C)])
        assert all(_bits(a, b) for a, b in zip(got, one))                 # C views in one call == C single-view calls, bit for bit
    ref = [t.double() for t in start]
    terms = torch.zeros(N, dtype=torch.float64)
    for v in range(C):
        _restate_accumulate(ref, xg[v], radii[v], float(max(H, W)))
        vis = radii[v] > 0
        terms[vis] += torch.sqrt(xg[v].double()[vis, 0] ** 2 + xg[v].double()[vis, 1] ** 2)
    assert torch.equal(got[1].double(), ref[1])                           # counts exact
    never = (radii > 0).sum(0) == 0
    assert never.any() or N == 1
    for k in range(3):
        assert _bits(got[k][never], start[k][never])                      # untouched
    seen = ~never
    if seen.any():
        # start value + per term 4 eps of the running sum (<= start + all terms)
        bar = 4 * EPS * (C * (start[0].double() + terms))[seen]
        within(f"accumulate grad_norm_sum N={N} C={C} (x bar)", ((got[0].double() - ref[0]).abs()[seen] / bar).max(), 1.0)
        within(f"accumulate max_2dsize N={N} C={C} (x bar)", ((got[2].double() - ref[2]).abs()[seen] / (2 * EPS * ref[2][seen])).max(), 1.0)


# ------------------------------------------------------------------------------------------------------------ plan + apply
@pytest.mark.parametrize("ns,N", [(ns, N) for ns in (2, 3) for N in SIZES + (SCAN_CHUNK if ns == 2 else ())])
def test_plan_apply_mixed(N, ns):
    P, stats = _population(N, seed=N + ns)
    mom = _moments(P, seed=N)
    ref, outs, wm, wsc = _run_plan_apply(P, stats, mom, ns)
    if N >= 16:
        a = ref["action"][:12].tolist()
        assert a == [KEEP, SPLIT | EMIT_SPLIT, KEEP | DUP | EMIT_DUP, BELOW_ALPHA, TOO_BIG, ON_SCREEN, SPLIT | TOO_BIG, DUP | BELOW_ALPHA,
                     SPLIT | DUP | EMIT_SPLIT | EMIT_DUP, KEEP, SPLIT | EMIT_SPLIT | TOO_BIG, SPLIT | BELOW_ALPHA], a
    if ref["n_split_src"]:
        within(f"child means N={N} ns={ns} (x 16 eps bar)", wm, 1.0)
        within(f"child scales N={N} ns={ns} (x bar)", wsc, 1.0)


def test_plan_apply_edge_populations():
    N, ns = 1000, 2
    # nothing to do: outputs equal inputs bit for bit
    P, stats = _population(N, seed=1, kind="quiet")
    mom = _moments(P, seed=2)
    ref, outs, _, _ = _run_plan_apply(P, stats, mom, ns)
    assert ref["counts"] == [N, 0, 0, N, 0]
    for t, k in enumerate(NAMES):
        assert _bits(outs[0][t], P[k]) and _bits(outs[1][t], mom[0][k]) and _bits(outs[2][t], mom[1][k])
    # everything culled: n_out == 0, empty tensors
    P, stats = _population(N, seed=3, kind="dead")
    ref, outs, _, _ = _run_plan_apply(P, stats, _moments(P, seed=4), ns)
    assert ref["counts"][:4] == [0, 0, 0, 0] and ref["counts"][4] >= N and all(t.shape[0] == 0 for t in outs[0])
    # no visible Gaussian: nothing is high, whatever the sums hold
    P, stats = _population(N, seed=5, kind="unseen")
    ref, outs, _, _ = _run_plan_apply(P, stats, _moments(P, seed=6), ns)
    assert ref["counts"][1] == 0 and ref["counts"][2] == 0 and not bool((ref["action"] & (SPLIT | DUP)).any())
    # optimizers without state: no moments at all, and moments of some tensors only
    P, stats = _population(N, seed=7)
    _run_plan_apply(P, stats, (None, None), ns)
    m, v = _moments(P, seed=8)
    for k in ("means", "features_rest"):
        m[k] = None; v[k] = None
    _run_plan_apply(P, stats, (m, v), ns)
    # cull only (no statistics at all), with and without the scale test; the smaller SH blocks
    for by_scale in (False, True):
        ref, _, _, _ = _run_plan_apply(P, None, _moments(P, seed=9), ns, densify=False, split_by_screen=False, cull_by_scale=by_scale,
                                       cull_by_screen=False)
        assert ref["counts"][1] == ref["counts"][2] == 0 and 0 < ref["counts"][0] < N
    for rest_k in (0, 3, 8):
        P, stats = _population(300, seed=10 + rest_k, rest_k=rest_k)
        _run_plan_apply(P, stats, _moments(P, seed=11), 4)


def test_refine_argument_checks():
    L = _lib(); lib = L.lib()
    P, stats = _population(64, seed=1)
    for ns in (0, 5, -1):
        rc, _, _, _ = _plan(P, stats, True, ns, True, True, True)
        assert rc == -1 and b"n_split_samples" in lib.gc_last_error_string()
    big = (1 << 31) // 45 // 4 + 1                                         # N * 45 * (2 + 2) reaches 2^31: refused before any launch or pointer use
    assert lib.gc_refine_plan_workspace_bytes(L.i64(big)) > 0
    one = torch.zeros(8, device=DEV)
    args = [L.ptr(one)] * 5 + [L.i32(1), L.i32(2)] + [L.f32(1.0)] * 3 + [L.i32(1), L.f32(1.0), L.f32(1.0), L.i32(1), L.f32(1.0), L.i32(1), L.f32(1.0)]
    import ctypes as C
    assert lib.gc_refine_plan(L.i64(big), *args, L.ptr(one), L.ptr(one), L.ptr(one), L.ptr(one), C.c_size_t(1 << 40), L.stream_ptr()) == -1
    assert b"2^31" in lib.gc_last_error_string()
    assert lib.gc_refine_accumulate_views(L.i64(1 << 30), L.i32(1), L.ptr(one), L.ptr(one), L.f32(1.0), L.ptr(one), L.ptr(one), L.ptr(one),
                                          L.stream_ptr()) == -1
    # N = 0: success, nothing launched, nothing written
    counts = torch.full((5,), -7, dtype=torch.int32, device=DEV)
    assert lib.gc_refine_plan(L.i64(0), *args, L.ptr(one), L.ptr(one), L.ptr(counts), L.ptr(one), C.c_size_t(0), L.stream_ptr()) == 0
    assert lib.gc_refine_accumulate_views(L.i64(0), L.i32(1), None, None, L.f32(1.0), None, None, None, L.stream_ptr()) == 0
    assert lib.gc_refine_reset_opacity(L.i64(0), L.f32(0.0), None, None, None, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert counts.tolist() == [-7] * 5


# ------------------------------------------------------------------------------------------------------------ reset
@pytest.mark.parametrize("N", [1, 257, 70001])
def test_reset_opacity(N):
    from gaussctrl_amd import refine
    L = _lib(); lib = L.lib()
    thresh = 0.1
    want = torch.logit(torch.tensor(2.0 * thresh, dtype=torch.float32))
    assert refine.reset_logit(thresh) == float(want)
    g = torch.Generator().manual_seed(N)
    op = torch.randn(N, 1, generator=g) * 3
    m, v = torch.randn(N, 1, generator=g), torch.rand(N, 1, generator=g)
    d = [on_device(t, DEV) for t in (op, m, v)]
    L.check(lib.gc_refine_reset_opacity(L.i64(N), L.f32(refine.reset_logit(thresh)), L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.stream_ptr()), "reset")
    got = [t.cpu() for t in d]
    over = op > want
    assert _bits(got[0][over], want.expand(int(over.sum()))) and _bits(got[0][~over], op[~over])          # clamp value exact, the rest untouched
    assert _bits(got[1], torch.zeros_like(m)) and _bits(got[2], torch.zeros_like(v))
    d = on_device(op, DEV)                                                  # without moments
    L.check(lib.gc_refine_reset_opacity(L.i64(N), L.f32(refine.reset_logit(thresh)), L.ptr(d), None, None, L.stream_ptr()), "reset")
    assert _bits(d.cpu(), got[0])


# ------------------------------------------------------------------------------------------------------------ the callback
def _scene(n=2000):
    from gaussctrl_amd import synthetic as syn
    from gaussctrl_amd.ns_compat import Cameras
    P = syn.make_gaussians(n, seed=21, scale_mean=0.05)
    c2ws = syn.make_cameras(4, seed=22)
    return P, Cameras(c2ws, 60.0, 60.0, 32.0, 32.0, 64, 64)


def _train(refine_on_device, steps=42):
    """a stand-alone model, FusedAdam per group, the built-in trainer's iteration order, a schedule shrunk into ~40 steps"""
    from gaussctrl_amd.gc_config import build_optimizers
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.gc_trainer import TrainingCallbackAttributes
    P, cams = _scene()
    cfg = GaussCtrlModelConfig(background_color="black", refine_on_device=refine_on_device, refine_every=5, reset_alpha_every=3, warmup_length=4,
                               stop_split_at=30, stop_screen_size_at=27, densify_grad_thresh=1e-7, densify_size_thresh=0.05,
                               cull_scale_thresh=0.12, cull_alpha_thresh=0.1, sh_degree_interval=1)
    model = GaussCtrlModel(cfg, params=P, device=DEV)
    model.train()
    target_model = GaussCtrlModel(GaussCtrlModelConfig(background_color="black", sh_degree_interval=1), params={k: v.copy() for k, v in P.items()}, device=DEV)
    with torch.no_grad():
        target_model.features_dc += 0.3
        targets = [target_model.get_outputs_for_camera(cams[i])["rgb"].clone() for i in range(4)]
    opts = build_optimizers(model)
    cbs = model.get_training_callbacks(TrainingCallbackAttributes(optimizers=opts, grad_scaler=None, pipeline=None))
    return model, cams, targets, opts, cbs, steps


def _iteration(model, cams, targets, opts, step):
    for o in opts.values():
        o.zero_grad(set_to_none=True)
    out = model.get_outputs(cams[step % 4])
    loss = model.get_loss_dict(out, {"image": targets[step % 4]})["main_loss"]
    loss.backward()
    for o in opts.values():
        o.step()
    return float(loss.detach())


def _nudge(model, state, c):
    """Move what sits within 2e-3 (relative) of a threshold 1 % (scales, gradient sums) or ~4 % (alpha) away, in float32, on the model and the
    statistics themselves: trained values land anywhere, and the count comparison below must not hang on a float32 / float64 knife edge."""
    with torch.no_grad():
        for thr in (c.densify_size_thresh, c.cull_scale_thresh, 1.6 * c.cull_scale_thresh):
            smax = model.scales.exp().max(dim=-1).values
            model.scales.data[((smax - thr).abs() / thr) < 2e-3] += 0.01
        a = torch.sigmoid(model.opacities.data)
        model.opacities.data[((a - c.cull_alpha_thresh).abs() / c.cull_alpha_thresh) < 2e-3] += 0.05
        if state.grad_norm_sum is not None:
            avg = state.grad_norm_sum / state.vis_count.clamp(min=1) * 0.5 * 64.0
            state.grad_norm_sum[((avg - c.densify_grad_thresh).abs() / c.densify_grad_thresh) < 2e-3] *= 1.01


def test_refine_callback_run():
    from gaussctrl_amd import refine
    from gaussctrl_amd.gc_trainer import RefineCallback, StepCallback
    model, cams, targets, opts, cbs, steps = _train(True)
    assert [type(c) for c in cbs] == [StepCallback, RefineCallback]
    step_cb, rcb = cbs
    rcb.num_train_data = 2
    c = model.config
    seen, sizes = set(), [model.num_points]
    for step in range(steps):
        step_cb.run_callback_at_location(step, "before_train_iteration")
        loss = _iteration(model, cams, targets, opts, step)
        assert math.isfinite(loss)
        sch = refine.schedule(c, step, 2)
        if not sch.refine:
            rcb.run_callback_at_location(step, "after_train_iteration")
            assert model.num_points == sizes[-1]
            continue
        # this step's statistics go in here, so that the inputs can be moved off the thresholds and copied for the restatement; the callback's
        # own accumulate then finds no gradient and the rest of it runs as in training
        if step < c.stop_split_at:
            rcb.state.accumulate(model)
        model._aux.xys_grad = None
        _nudge(model, rcb.state, c)
        n_before = model.num_points
        Pc = {k: getattr(model, k).detach().cpu().clone() for k in NAMES}
        st = None if rcb.state.grad_norm_sum is None else tuple(t.cpu().clone() for t in (rcb.state.grad_norm_sum, rcb.state.vis_count, rcb.state.max_2dsize))
        assert st is not None or not sch.densify
        steps_before = {g: [o.state[p]["step"] for p in o.param_groups[0]["params"]] for g, o in opts.items()}
        th = dict(max_dim=64.0, densify_grad_thresh=c.densify_grad_thresh, densify_size_thresh=c.densify_size_thresh,
                  split_screen_size=c.split_screen_size, cull_alpha_thresh=c.cull_alpha_thresh, cull_scale_thresh=c.cull_scale_thresh,
                  cull_screen_size=c.cull_screen_size)
        want, ref = n_before, None
        if sch.densify or sch.cull_only:
            ref = _restate(Pc, st if sch.densify else None, th, sch.densify, c.n_split_samples, sch.densify and sch.by_screen, sch.cull_by_scale,
                           sch.densify and sch.cull_by_scale and sch.by_screen)
            _guard(ref)
            want = ref["counts"][3]
        torch.manual_seed(step)
        rcb.run_callback_at_location(step, "after_train_iteration")
        seen.add((sch.densify, sch.cull_only, sch.reset))
        assert model.num_points == want, (step, model.num_points, want)
        sizes.append(want)
        if ref is not None:
            assert [rcb.state.last[k] for k in ("n_survivors", "n_split_src", "n_dup_src", "n_out", "n_below_alpha")] == ref["counts"]
            if ref["counts"][1]:                              # the children's means come from torch.randn under the seed set above
                torch.manual_seed(step)
                smp = torch.randn(c.n_split_samples * ref["counts"][1], 3, device=DEV).cpu()
                spl = ref["kind"] == 1
                m64, v = _child_means64(Pc, ref["src"][spl], smp)
                bar = 16 * EPS * (Pc["means"][ref["src"][spl]].double().abs().amax(-1) + v.abs().amax(-1))
                assert bool(((model.means.detach().cpu()[spl].double() - m64).abs().amax(-1) <= bar).all())
            added = ref["counts"][1] + ref["counts"][2] > 0
            if want != n_before or added:
                keep = getattr(model, "_cull_keep", None)
                if added:                                     # the sharded-Adam path gets a mask only from a pure cull
                    assert keep is None
                else:
                    assert keep is not None and keep.numel() == n_before and int(keep.sum()) == want
                    model._cull_keep = None
        if sch.reset:
            lim = refine.reset_logit(c.cull_alpha_thresh)
            assert float(model.opacities.detach().max()) <= lim
            s_ = opts["opacity"].state[model.opacities]
            assert float(s_["exp_avg"].abs().max()) == 0.0 and float(s_["exp_avg_sq"].abs().max()) == 0.0
        assert rcb.state.grad_norm_sum is None                               # statistics cleared
        rebuilt = ref is not None and (want != n_before or ref["counts"][1] + ref["counts"][2] > 0)
        for gname, o in opts.items():
            assert len(o.state) == 1
            for k, p in enumerate(o.param_groups[0]["params"]):
                assert p.shape[0] == model.num_points and (p.grad is None or not rebuilt)
                s_ = o.state[p]
                assert s_["exp_avg"].shape == p.shape and s_["exp_avg_sq"].shape == p.shape
                assert s_["step"] == steps_before[gname][k]
        model.eval()
        with torch.no_grad():
            img = model.get_outputs(cams[0])["rgb"]
        model.train()
        assert bool(torch.isfinite(img).all())
    # a densify, a reset and a post-stop_split_at cull fell inside the run; the set grew at a densify step
    assert {(True, False, False), (False, False, True), (False, True, False)} <= seen, seen
    assert rcb.n_added > 0 and max(sizes) > sizes[0], sizes


def test_callbacks_without_the_switch_are_the_parents():
    """refine_on_device = False: [StepCallback, CullCallback], and the same run culls what CullCallback's own rule culls"""
    from gaussctrl_amd.gc_trainer import CullCallback, StepCallback
    model, cams, targets, opts, cbs, steps = _train(False, steps=12)
    assert [type(c) for c in cbs] == [StepCallback, CullCallback]
    model.config.stop_split_at = 5                    # CullCallback acts from here on (every refine_every = 5 steps)
    counts = []
    for step in range(steps):
        for cb in cbs:
            cb.run_callback_at_location(step, "before_train_iteration")
        _iteration(model, cams, targets, opts, step)
        with torch.no_grad():
            culls = (torch.sigmoid(model.opacities) < model.config.cull_alpha_thresh).squeeze(-1)
            if step > model.config.refine_every * model.config.reset_alpha_every:
                culls |= torch.exp(model.scales).max(dim=-1).values > model.config.cull_scale_thresh
            want = model.num_points - int(culls.sum()) if (step >= 5 and step % 5 == 0) else model.num_points
        for cb in cbs:
            cb.run_callback_at_location(step, "after_train_iteration")
        assert model.num_points == want
        counts.append(model.num_points)
    assert not hasattr(model, "_refine_state")
