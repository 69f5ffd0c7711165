"""The training-step kernels (gaussctrl_amd/csrc/train_step.hip) against float64: fused L1+SSIM, depth L1, fused Adam.

References and bars: tests/_train_step_ref.py (tests/test_train_step_ref_cpu.py holds them to the oracle and shows that each bar can fail).
No bar here is a constant taken from a kernel's output: each is derived (roundings counted in the helper's docstrings) or computed from the
float32 / float64 oracle on the same inputs.

  L1+SSIM   smooth renders with a small residual, flat 0.0 / 1.0 regions with exact ties, pred == target, and uniform noise; C = 1, 3, 4;
            images below the 11 x 11 window, one SSIM pixel, one pixel more than the window, one 16 x 16 tile, tiles + 1; both window modes;
            lambda 0, 0.2, 1; the batched form per view against float64 (not against the single-image form); the refusals of the C ABI
  Adam      parameter AND both moments per element, gradient sizes from exactly 0 over 1e-20 (against eps 1e-15) to 1e18 in one tensor,
            steps 1, 2, 10 and 30001 (a resumed checkpoint), n around the 16-byte chunks, and the second trip of the grid-stride loops of
            k_adam and k_adam_rows (n > 2048 workgroups x 256 lanes x 4 floats)
  depth L1  2 and 64 per-workgroup partials folded by k_depth_l1_grad, invalid pixels at the ends of the workgroups' ranges
"""
import copy

import numpy as np
import pytest
import torch

import _train_step_ref as R
from _margins import within
from _redzone import on_device

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GC_EINVAL, GC_ENOSPC = -1, -3
SIZES = R.PADDED_ONLY + R.BOTH_MODES
HYPER = ((1.6e-4, 0.9, 0.999, 1e-15), (5e-3, 0.9, 0.999, 1e-15), (2.5e-3, 0.9, 0.999, 1e-8), (1.6e-4, 0.5, 0.9, 1e-15))
SWEEP = 2048 * 256 * 4                   # floats one sweep of the Adam launches covers


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return on_device(t if dtype is None else t.to(dtype), DEV)


# ------------------------------------------------------------------------------------------------------------------------ L1 + SSIM
def _loss_and_grad(pred, tgt, lam, valid):
    from gaussctrl_amd.train_ops import l1_ssim_loss
    p = on_device(pred, DEV).requires_grad_(True)
    loss = l1_ssim_loss(p, on_device(tgt, DEV), lam, valid_window=valid)
    loss.backward()
    return float(loss.detach()), p.grad


def _hold(case, loss, grad, label):
    print(f"{label}: gradient {R.grad_measure(grad, case['grad64']):.4g} / {case['grad_bar']:.4g} (float32 oracle {case['e32']:.4g}), "
          f"loss {abs(loss - case['loss64']):.4g} / {case['loss_bar']:.4g}")
    within(f"L1+SSIM gradient, max |g - g64| n, {label}", R.grad_measure(grad, case["grad64"]), case["grad_bar"])
    within(f"L1+SSIM loss, |l - l64|, {label}", abs(loss - case["loss64"]), case["loss_bar"])


@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("H,W", SIZES)
def test_l1_ssim_vs_float64(H, W, C):
    """l1_ssim_loss (value and gradient) against the float64 oracle on every image kind and window mode; two runs give the same gradient
    bits (the gradient path has no atomics; the loss sums are float atomics and are only held to their bar)"""
    for kind in R.KINDS:
        for valid in R.modes_of(H, W):
            case = R.ssim_case(kind, H, W, C, valid)
            loss, grad = _loss_and_grad(case["pred"], case["tgt"], 0.2, valid)
            _hold(case, loss, grad, f"{kind} {H}x{W}x{C} {'valid' if valid else 'padded'}")
            loss2, grad2 = _loss_and_grad(case["pred"], case["tgt"], 0.2, valid)
            assert torch.equal(_bits(grad), _bits(grad2)), (kind, valid)
            within(f"L1+SSIM loss, second run, {kind} {H}x{W}x{C} {'valid' if valid else 'padded'}", abs(loss2 - case["loss64"]), case["loss_bar"])


@pytest.mark.parametrize("valid", [True, False])
def test_l1_ssim_lambda_0_and_1(valid):
    """lambda = 1 (SSIM alone) to the same bars; lambda = 0: every gradient element within 1 ulp of sign(pred - target) * float32(1 / n),
    exactly 0 on ties (`flat` has a quarter of exact ties)"""
    H, W, C = 17, 33, 3
    for lam in (0.0, 1.0):
        case = R.ssim_case("residual", H, W, C, valid, lam)
        loss, grad = _loss_and_grad(case["pred"], case["tgt"], lam, valid)
        _hold(case, loss, grad, f"residual {H}x{W}x{C} {'valid' if valid else 'padded'} lambda {lam:g}")
    for kind in ("residual", "flat"):
        case = R.ssim_case(kind, H, W, C, valid, 0.0)
        _, grad = _loss_and_grad(case["pred"], case["tgt"], 0.0, valid)
        got = grad.cpu().numpy().astype(np.float64)
        sign = np.sign(case["pred"].numpy().astype(np.float64) - case["tgt"].numpy().astype(np.float64))
        want = sign * float(np.float32((1.0 - 0.0) / case["n"]))
        assert np.all(got[sign == 0] == 0.0) and ((sign == 0).sum() > 0) == (kind == "flat")
        within(f"L1 gradient at lambda 0, ulps, {kind} {'valid' if valid else 'padded'}",
               (np.abs(got - want) / np.spacing(np.float32(1.0 / case["n"]))).max(), 1.0)


def test_l1_ssim_views_vs_float64_per_image():
    """l1_ssim_loss_views, B = 3 (uniform, flat, equal) with per-view weights: each view's loss and gradient to the single-image bars of its
    own kind -- a slot line or a workspace slice that bleeds into the neighbouring view shows here"""
    from gaussctrl_amd.train_ops import l1_ssim_loss_views
    H, W, C = 17, 33, 3
    kinds, weights = ("uniform", "flat", "equal"), (0.5, 2.0, 0.25)            # powers of two: grad / weight is exact
    for valid in (True, False):
        cases = [R.ssim_case(k, H, W, C, valid) for k in kinds]
        x = on_device(torch.stack([c["pred"] for c in cases]), DEV).requires_grad_(True)
        y = on_device(torch.stack([c["tgt"] for c in cases]), DEV)
        lv = l1_ssim_loss_views(x, y, 0.2, valid_window=valid)
        (lv * on_device(torch.tensor(weights), DEV)).sum().backward()
        for b, (kind, case) in enumerate(zip(kinds, cases)):
            _hold(case, float(lv[b].detach()), x.grad[b] / weights[b], f"view {b} ({kind}) of 3, {H}x{W}x{C} {'valid' if valid else 'padded'}")


def test_l1_ssim_abi_edges():
    """gc_l1_ssim_fwd_bwd[_views] directly: grad_scale 0.5 and 4 scale the gradient bit for bit; valid-window SSIM of an image with H = 10 or
    W = 10, 65536 image planes, and a workspace one byte short are refused before anything is launched (no output byte changes)"""
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    H, W, C = 17, 33, 3
    case = R.ssim_case("residual", H, W, C, True)
    p, t = on_device(case["pred"], DEV), on_device(case["tgt"], DEV)

    def run(grad_scale, H=H, W=W, C=C, valid=1, short=0, views=0, p=p, t=t):
        nbytes = lib.gc_l1_ssim_views_workspace_bytes(views, H, W, C) if views else lib.gc_l1_ssim_workspace_bytes(H, W, C)
        ws = torch.full((nbytes // 4 + 1,), 7.0, dtype=torch.float32, device=DEV)
        sums = torch.full((max(views, 1), 2), 7.0, dtype=torch.float32, device=DEV)
        v = torch.full((p.numel(),), 7.0, dtype=torch.float32, device=DEV)
        tail = (H, W, C, 0.2, grad_scale, valid, L.ptr(sums), L.ptr(v), L.ptr(ws), nbytes - short, L.stream_ptr())
        rc = lib.gc_l1_ssim_fwd_bwd_views(views, L.ptr(p), L.ptr(t), *tail) if views else lib.gc_l1_ssim_fwd_bwd(L.ptr(p), L.ptr(t), *tail)
        torch.cuda.synchronize()
        untouched = all(bool((b == 7.0).all()) for b in (ws, sums, v))
        return rc, v, untouched

    rc, v1, untouched = run(1.0)
    assert rc == 0 and not untouched
    within("L1+SSIM gradient through the C ABI, max |g - g64| n", R.grad_measure(v1.reshape(H, W, C), case["grad64"]), case["grad_bar"])
    for scale in (0.5, 4.0):
        rc, v, _ = run(scale)
        assert rc == 0 and torch.equal(_bits(v), _bits(v1 * scale)), scale
    refused = {"H = 10": dict(H=10), "W = 10": dict(W=10), "views, H = 10": dict(H=10, views=1)}
    for name, kw in refused.items():
        assert run(1.0, **kw)[::2] == (GC_EINVAL, True), name
    assert run(1.0, H=10, valid=0)[0] == 0 and run(1.0, H=11, W=11)[0] == 0            # (the padded mode takes any size; 11 x 11 is the smallest valid one)
    planes = on_device(torch.rand(65536), DEV)
    assert run(1.0, H=1, W=1, C=65536, valid=0, p=planes, t=planes)[::2] == (GC_EINVAL, True)
    assert run(1.0, H=1, W=1, C=256, valid=0, views=256, p=planes, t=planes)[::2] == (GC_EINVAL, True)
    assert run(1.0, H=1, W=1, C=65535, valid=0, p=planes, t=planes)[0] == 0
    assert run(1.0, short=1)[::2] == (GC_ENOSPC, True) and run(1.0, short=1, views=2, H=8, valid=0)[::2] == (GC_ENOSPC, True)
    assert b"workspace" in lib.gc_last_error_string()


# ------------------------------------------------------------------------------------------------------------------------------- Adam
def _adam_step(arrays, n, lr, b1, b2, eps, step):
    """gc_adam_step on fresh device copies of the float32 arrays (p, g, m, v) -> (p, m, v) as numpy"""
    from gaussctrl_amd import _lib as L
    p, g, m, v = (_dev(a) for a in arrays)
    L.check(L.lib().gc_adam_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), n, lr, b1, b2, eps, step, L.stream_ptr()), "gc_adam_step")
    return tuple(x.cpu().numpy() for x in (p, m, v))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 7, 1023, 1024, 1025])
def test_adam_vs_float64(n):
    """gc_adam_step against adam_ref: parameter, exp_avg and exp_avg_sq per element to the derived bars of _train_step_ref.adam_shares, at
    steps 1, 2, 10 from zero moments and step 30001 from a checkpoint's, four hyper-parameter sets, gradient sizes 0 .. 1e18 element by
    element.  Elements with g = 0 and zero moments keep the bits of p, m and v."""
    for (lr, b1, b2, eps) in HYPER:
        for step in (1, 2, 10, 30001):
            p, g, m, v = R.adam_inputs(n, 1000 * n + step, moments=step > 10)
            got = _adam_step((p, g, m, v), n, lr, b1, b2, eps, step)
            ref = R.adam_ref(p, g, m, v, lr, b1, b2, eps, step)
            shares = R.adam_shares(got, p, ref, lr, b1, step)
            print(f"n {n} lr {lr:g} betas ({b1:g}, {b2:g}) eps {eps:g} step {step}: {shares}")
            for what, share in shares.items():
                within(f"Adam {what}, worst share of the per-element bar, lr {lr:g} betas ({b1:g}, {b2:g}) eps {eps:g} step {step}", share, 1.0)
            still = (g == 0) & (m == 0) & (v == 0)
            for was, now in zip((p, m, v), got):
                assert np.array_equal(was[still].view(np.int32), now[still].view(np.int32))
            assert n < 8 or not np.array_equal(got[0][~still], p[~still])


@pytest.mark.parametrize("step", [1, 30001])
def test_adam_second_sweep_vs_torch(step):
    """n = 2 097 159: the smallest n with a scalar tail whose 16-byte chunks need a second trip of k_adam's grid-stride loop (n4 = 524 289 >
    2048 x 256).  Every element against torch.optim.Adam in float64 at the python-double hyper-parameters: the kernel is exact Adam at the
    float32-rounded betas, 1.29e-5 from torch's through 1 - beta2, and float32's own roundings (below 1e-6 relative on gradients of one size)
    fit beside that in 2e-5; the parameter additionally gets the half ulp of its own rounding.  An element the second trip skipped keeps zero
    moments and fails."""
    n = SWEEP + 7
    assert (n // 4) > 2048 * 256 and n % 4 == 3
    lr, b1, b2, eps = HYPER[0]
    r = np.random.default_rng(step)
    p, g = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    m = (0.3 * r.standard_normal(n)).astype(np.float32) if step > 1 else np.zeros(n, np.float32)
    v = r.uniform(0.5, 1.5, n).astype(np.float32) if step > 1 else np.zeros(n, np.float32)
    gp, gm, gv = (a.astype(np.float64) for a in _adam_step((p, g, m, v), n, lr, b1, b2, eps, step))
    x = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([x], lr=lr, betas=(b1, b2), eps=eps)
    if step > 1:
        opt.state[x] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                            exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
    x.grad = torch.from_numpy(g.astype(np.float64))
    opt.step()
    tp, tm, tv = x.detach().numpy(), opt.state[x]["exp_avg"].numpy(), opt.state[x]["exp_avg_sq"].numpy()
    mag = np.abs(0.9 * m) + np.abs(0.1 * g)
    scale = lr / (1.0 - b1 ** step) * mag / (np.sqrt(tv) / np.sqrt(1.0 - b2 ** step) + eps)       # the update's size by its operands, as in adam_shares
    within("Adam exp_avg vs torch float64, relative to its operands, second sweep", (np.abs(gm - tm) / mag).max(), 2e-5)
    within("Adam exp_avg_sq vs torch float64, relative, second sweep", (np.abs(gv - tv) / tv).max(), 2e-5)
    within("Adam parameter vs torch float64, share of 2e-5 of the update + the parameter's half ulp, second sweep",
           (np.abs(gp - tp) / (2e-5 * scale + 0.5 * np.maximum(R.ulp32(p), R.ulp32(tp)))).max(), 1.0)


@pytest.mark.parametrize("rows,rf", [(699053, 3), (46604, 45)])
def test_adam_rows_second_sweep(rows, rf):
    """tests/test_edit_trace_gpu.py::test_adam_step_rows at a size that leaves the first sweep of k_adam_rows: selected rows carry the bits of
    gc_adam_step on a copy, every other row of p, m and v keeps its bits"""
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    n = rows * rf
    assert n // 4 > 2048 * 256
    g = torch.Generator().manual_seed(rows + rf)
    patterns = {"alternating": _dev(torch.arange(rows) % 2, torch.uint8), "random 10 %": _dev(torch.rand(rows, generator=g) < 0.1, torch.uint8)}
    hyper = (1.6e-4, 0.9, 0.999, 1e-15)
    for name, sel in patterns.items():
        p = _dev(torch.randn(rows, rf, generator=g)); m = _dev(torch.randn(rows, rf, generator=g) * 1e-3)
        v = _dev(torch.rand(rows, rf, generator=g) * 1e-6)
        on = sel.bool()
        for step in (1, 2):
            grad = _dev(torch.randn(rows, rf, generator=g) * 1e-2)
            before = [t.clone() for t in (p, m, v)]
            ref = [on_device(t, DEV) for t in (p, m, v)]
            L.check(lib.gc_adam_step(L.ptr(ref[0]), L.ptr(grad), L.ptr(ref[1]), L.ptr(ref[2]), n, *hyper, step, L.stream_ptr()), "gc_adam_step")
            L.check(lib.gc_adam_step_rows(L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), rows, rf, L.ptr(sel), *hyper, step, L.stream_ptr()),
                    "gc_adam_step_rows")
            for what, got, r, b in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), ref, before):
                assert torch.equal(_bits(got[on]), _bits(r[on])), (name, step, what, "selected rows")
                assert torch.equal(_bits(got[~on]), _bits(b[~on])), (name, step, what, "unselected rows")
                assert not torch.equal(_bits(r), _bits(b)), (name, step, what)
        assert name != "alternating" or bool(on[SWEEP // rf:].any())          # a selected row that only the second trip reaches


def test_fused_adam_groups_skips_and_state_dict():
    """FusedAdam: two parameter groups (their own lr and eps), a parameter without a gradient, a non-contiguous gradient; three steps, each
    against adam_ref from the state before it; the skipped parameter keeps its bits and gets no state; state_dict() after step 2 loaded
    into a fresh FusedAdam gives step 3 the bits of the uninterrupted run in p, exp_avg and exp_avg_sq"""
    from gaussctrl_amd.train_ops import FusedAdam
    g = torch.Generator().manual_seed(9)
    shapes = ((37, 3), (5, 15, 3), (11,), (6, 45))
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * 10.0 ** (it - 1) for s in shapes] for it in range(3)]
    groups_of = lambda ps: [dict(params=[ps[0], ps[2]], lr=1.6e-4, eps=1e-15), dict(params=[ps[1], ps[3]], lr=5e-3, eps=1e-8)]
    hyper = {0: (1.6e-4, 1e-15), 2: (1.6e-4, 1e-15), 1: (5e-3, 1e-8), 3: (5e-3, 1e-8)}

    def set_grads(ps, it):
        for k, x in enumerate(ps):
            x.grad = None if k == 2 else on_device(grads[it][k], DEV)
        ps[3].grad = on_device(grads[it][3].t().contiguous(), DEV).t()          # [6,45] values, strides (1, 6)
        assert not ps[3].grad.is_contiguous() and torch.equal(ps[3].grad.cpu(), grads[it][3])

    ps = [torch.nn.Parameter(on_device(x, DEV)) for x in init]
    opt = FusedAdam(groups_of(ps))
    saved = None
    for it in range(3):
        set_grads(ps, it)
        before = [(x.detach().cpu().numpy().ravel(), *(opt.state[x][k].cpu().numpy().ravel() if opt.state[x] else np.zeros(x.numel(), np.float32)
                                                         for k in ("exp_avg", "exp_avg_sq"))) for x in ps]
        opt.step()
        for k, x in enumerate(ps):
            if k == 2:
                assert torch.equal(_bits(x.detach()), _bits(on_device(init[2], DEV))) and not opt.state[x]
                continue
            lr, eps = hyper[k]
            p0, m0, v0 = before[k]
            ref = R.adam_ref(p0, grads[it][k].numpy().ravel(), m0, v0, lr, 0.9, 0.999, eps, it + 1)
            got = tuple(t.detach().cpu().numpy().ravel() for t in (x, opt.state[x]["exp_avg"], opt.state[x]["exp_avg_sq"]))
            assert opt.state[x]["step"] == it + 1
            for what, share in R.adam_shares(got, p0, ref, lr, 0.9, it + 1).items():
                within(f"FusedAdam {what}, worst share of the per-element bar, parameter {k} step {it + 1}", share, 1.0)
        if it == 1:
            saved = (copy.deepcopy(opt.state_dict()), [x.detach().cpu() for x in ps])       # (state_dict holds the live tensors)
    ps2 = [torch.nn.Parameter(on_device(x, DEV)) for x in saved[1]]
    opt2 = FusedAdam(groups_of(ps2), lr=1.0, eps=1.0)
    opt2.load_state_dict(saved[0])
    set_grads(ps2, 2)
    opt2.step()
    for k, (a, b) in enumerate(zip(ps, ps2)):
        assert torch.equal(_bits(a.detach()), _bits(b.detach())), k
        assert bool(opt.state[a]) == bool(opt2.state[b]) == (k != 2)
        for key in (("exp_avg", "exp_avg_sq") if k != 2 else ()):
            assert torch.equal(_bits(opt.state[a][key]), _bits(opt2.state[b][key])), (k, key)


# --------------------------------------------------------------------------------------------------------------------------- depth L1
def _depth_l1(pred, target):
    """gc_depth_l1_fwd_bwd_views with grad_scale 1 -> ({sum, count} per view, gradient) as numpy"""
    from gaussctrl_amd import _lib as L
    B, H, W = pred.shape
    p, t = _dev(pred), _dev(target)
    nbytes = L.call("gc_depth_l1_views_workspace_bytes", B, H, W)
    ws = torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=DEV)
    sums = torch.empty(B, 2, dtype=torch.float32, device=DEV)
    v = torch.empty(B, H, W, dtype=torch.float32, device=DEV)
    L.call("gc_depth_l1_fwd_bwd_views", B, p, t, H, W, 1.0, sums, v, ws, nbytes)
    return sums.cpu().numpy(), v.cpu().numpy()


@pytest.mark.parametrize("empty_view", [0, 1])
@pytest.mark.parametrize("H,W", [(3, 683), (257, 512)])
def test_depth_l1_beyond_one_partial(H, W, empty_view):
    """B = 2 at hw = 2049 (two per-workgroup partials) and 131 584 (64, the cap), one view without a valid pixel: the fold of
    k_depth_l1_grad against float64.  Invalid pixels of every kind sit on the first and last elements of the workgroups' ranges."""
    hw = H * W
    nblk = min(64, (hw + 2047) // 2048)
    assert nblk == (2 if hw == 2049 else 64)
    r = np.random.default_rng(hw)
    pred = r.uniform(1.0, 6.0, size=(2, hw)).astype(np.float32)
    target = r.uniform(1.0, 6.0, size=(2, hw)).astype(np.float32)
    full = 1 - empty_view
    if empty_view == 0:
        pred[0] = 1000.0
    else:
        target[1] = np.where(np.arange(hw) % 2 == 0, np.float32(np.nan), np.float32(1000.0))
    pred[full, r.random(hw) < 0.1] = 1000.0
    # a workgroup's range: elements bx * 256 + lane + k * nblk * 256; its first and last lanes in the first, second and last trip
    stride = nblk * 256
    ends = sorted({i for bx in (0, 1, nblk - 1) for k in (0, 1, (hw - 1) // stride) for i in (bx * 256 + k * stride, bx * 256 + 255 + k * stride)
                   if i < hw} | {hw - 1, hw - 2})
    kinds = ("pred sentinel", "target sentinel", "both", "inf", "nan", "tie", "valid")
    for j, i in enumerate(ends):
        kind = kinds[j % len(kinds)]
        pred[full, i] = {"pred sentinel": 1000.0, "both": 1000.0, "inf": np.inf, "valid": 2.0}.get(kind, 3.0)
        target[full, i] = {"target sentinel": 1000.0, "both": 1000.0, "nan": np.nan, "tie": 3.0, "valid": 5.0}.get(kind, 4.0)
    pred, target = pred.reshape(2, H, W), target.reshape(2, H, W)
    sums, grad = _depth_l1(pred, target)
    with np.errstate(invalid="ignore"):
        valid, diff, cnt, want = R.depth_l1_ref(pred, target)
    assert cnt[empty_view] == 0 and 0.8 * hw < cnt[full] < hw and (diff[full][valid[full]] == 0).sum() >= 1
    assert np.array_equal(sums[:, 1].astype(np.int64), cnt), (sums[:, 1], cnt)
    got = sums[:, 0].astype(np.float64) / np.maximum(cnt, 1)
    assert sums[empty_view, 0] == 0.0
    within("depth L1 loss, relative", np.abs(got - want).max() / np.abs(want).max(), 1e-6)
    inv = (1.0 / np.maximum(cnt, 1)).astype(np.float32).astype(np.float64)
    wantg = np.sign(diff) * inv[:, None, None]
    gotg = grad.astype(np.float64)
    assert np.all(gotg[~valid] == 0.0) and np.all(gotg[diff == 0] == 0.0)
    within("depth L1 gradient, ulps of float32(1 / count)", (np.abs(gotg - wantg) / R.ulp32(inv)[:, None, None]).max(), 1.0)
    sums2, grad2 = _depth_l1(pred, target)                        # fixed-order fold: the same bits every time
    assert np.array_equal(sums.view(np.int32), sums2.view(np.int32)) and np.array_equal(grad.view(np.int32), grad2.view(np.int32))
