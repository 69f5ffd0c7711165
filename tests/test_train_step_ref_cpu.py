"""The references of tests/test_train_step_gpu.py (tests/_train_step_ref.py) against the project's oracle and torch, and proof that the bars
they set can fail.  Everything here runs on the CPU; no kernel is touched."""
import numpy as np
import pytest
import torch

import _train_step_ref as R

SSIM_CASES = [(H, W, C, valid) for (H, W) in R.PADDED_ONLY + R.BOTH_MODES for C in R.CHANNELS for valid in R.modes_of(H, W)]
HYPER = ((1.6e-4, 0.9, 0.999, 1e-15), (5e-3, 0.9, 0.999, 1e-15), (2.5e-3, 0.9, 0.999, 1e-8), (1.6e-4, 0.5, 0.9, 1e-15))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("valid", [True, False])
def test_ssim_map_mean_is_the_oracle_ssim(dtype, valid):
    """the mean of ssim_map has the bits of oracle/sd15_torch.py::ssim, and splat_loss_ref those of splat_loss"""
    from oracle import sd15_torch as sd
    for kind in ("uniform", "flat"):
        pred, tgt = R.make_images(kind, 44, 37, 3, seed=7)
        a, b = tgt.permute(2, 0, 1)[None].to(dtype), pred.permute(2, 0, 1)[None].to(dtype)
        m = R.ssim_map(a, b, valid, dtype)
        assert m.dtype == dtype and m.shape == ((1, 3, 34, 27) if valid else (1, 3, 44, 37))
        assert m.mean().item() == sd.ssim(a, b, valid=valid).item()
        loss, grad, _ = R.splat_loss_ref(pred, tgt, 0.2, valid, dtype)
        want = sd.splat_loss(pred.to(dtype), tgt.to(dtype), 0.2, valid=valid)
        assert loss.item() == want.item() and grad.dtype == dtype and grad.shape == pred.shape


def test_make_images():
    for kind in R.KINDS:
        for (H, W, C) in ((1, 1, 1), (5, 7, 4), (44, 37, 3)):
            pred, tgt = R.make_images(kind, H, W, C, seed=3)
            again = R.make_images(kind, H, W, C, seed=3)
            assert torch.equal(pred, again[0]) and torch.equal(tgt, again[1])
            for t in (pred, tgt):
                assert t.shape == (H, W, C) and t.dtype == torch.float32 and float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    pred, tgt = R.make_images("flat", 44, 37, 3, seed=3)
    assert float(tgt[:22, 12:].abs().max()) == 0.0 and bool((tgt[:, :12] == 1.0).all())
    assert torch.equal(pred[:11], tgt[:11]) and not torch.equal(pred[11:], tgt[11:])
    pred, tgt = R.make_images("equal", 44, 37, 3, seed=3)
    assert torch.equal(pred, tgt) and float(tgt.std()) > 0.05
    pred, tgt = R.make_images("residual", 44, 37, 3, seed=3)
    assert 0.005 < float((pred - tgt).std()) < 0.02


@pytest.mark.parametrize("H,W,C,valid", SSIM_CASES)
def test_ssim_gradient_bar_can_fail(H, W, C, valid):
    """a float64 oracle with sigma = 1.51, one with C2 = 0.033^2, and the other window mode each exceed the gradient bar of every image
    kind whose gradient is not zero"""
    for kind in ("uniform", "residual", "flat"):
        case = R.ssim_case(kind, H, W, C, valid)
        mutants = {"sigma 1.51": dict(valid=valid, sigma=1.51), "C2 0.033^2": dict(valid=valid, c2=0.033 ** 2)}
        if len(R.modes_of(H, W)) == 2:
            mutants["window mode swapped"] = dict(valid=not valid)
        for name, kw in mutants.items():
            _, grad, _ = R.splat_loss_ref(case["pred"], case["tgt"], 0.2, dtype=torch.float64, **kw)
            err = R.grad_measure(grad, case["grad64"])
            assert err > case["grad_bar"], (kind, name, err, case["grad_bar"])


def test_ssim_bars_hold_for_the_float32_oracle_itself():
    """by construction (4 x its own error); the `equal` bar is held by the float32 oracle too, and is far below a real SSIM gradient"""
    for (H, W, C, valid) in SSIM_CASES:
        for kind in R.KINDS:
            case = R.ssim_case(kind, H, W, C, valid)
            loss32, grad32, _ = R.splat_loss_ref(case["pred"], case["tgt"], 0.2, valid, torch.float32)
            assert R.grad_measure(grad32, case["grad64"]) <= case["grad_bar"], (kind, H, W, C, valid)
            assert abs(float(loss32) - case["loss64"]) <= case["loss_bar"], (kind, H, W, C, valid)
        res = R.ssim_case("residual", H, W, C, valid)
        _, ssim_grad, _ = R.splat_loss_ref(res["pred"], res["tgt"], 1.0, valid, torch.float64)
        assert case["grad_bar"] < 0.2 * float(ssim_grad.abs().max()) * case["n"], (H, W, C, valid)     # (case: the `equal` one)


def _torch_adam(p, grads, lr, b1, b2, eps, m=None, v=None, step0=0):
    """torch.optim.Adam in float64 at the python-double hyper-parameters, from the given state"""
    x = torch.nn.Parameter(torch.tensor(p, dtype=torch.float64))
    opt = torch.optim.Adam([x], lr=lr, betas=(b1, b2), eps=eps)
    if step0:
        opt.state[x] = dict(step=torch.tensor(float(step0)), exp_avg=torch.tensor(m, dtype=torch.float64), exp_avg_sq=torch.tensor(v, dtype=torch.float64))
    for g in grads:
        x.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
    return x.detach().numpy(), opt.state[x]["exp_avg"].numpy(), opt.state[x]["exp_avg_sq"].numpy()


@pytest.mark.parametrize("lr,b1,b2,eps", HYPER)
def test_adam_ref_is_torch_adam_at_the_rounded_betas(lr, b1, b2, eps):
    """The kernel is exact Adam at the float32-ROUNDED betas: adam_ref gets those, torch.optim.Adam the python doubles.  They differ by the
    rounding of beta2, (1 - float32(0.999)) / (1 - 0.999) - 1 = -1.29e-5, so ten steps of updates agree to 2e-5 relative (and one step from
    a checkpoint at step 30000)."""
    if b2 == 0.999:
        assert abs((1 - float(np.float32(0.999))) / (1 - 0.999) - 1 + 1.29e-5) < 1e-7
    n = 64
    p0, _, m0, v0 = R.adam_inputs(n, 5, moments=True)
    grads = [R.adam_inputs(n, 10 + k, moments=False)[1] for k in range(10)]
    for start, (m, v) in ((0, (np.zeros(n), np.zeros(n))), (30000, (m0, v0))):
        p, ms, vs = p0.astype(np.float64), np.asarray(m, np.float64), np.asarray(v, np.float64)
        steps = grads if start == 0 else grads[:1]
        for k, g in enumerate(steps):
            p, ms, vs, _, _ = R.adam_ref(p, g, ms, vs, lr, b1, b2, eps, start + k + 1)
        tp, tm, tv = _torch_adam(p0, steps, lr, b1, b2, eps, m, v, start)
        upd, tupd = p - p0, tp - p0
        assert np.all(np.abs(upd - tupd) <= 2e-5 * np.abs(tupd) + 1e-300), float(np.max(np.abs(upd - tupd) / (np.abs(tupd) + 1e-300)))
        assert np.all(np.abs(ms - tm) <= 2e-5 * np.abs(tm)) and np.all(np.abs(vs - tv) <= 2e-5 * np.abs(tv))


@pytest.mark.parametrize("step", [1, 2, 10, 30001])
@pytest.mark.parametrize("lr,b1,b2,eps", HYPER)
def test_adam_bars_hold_for_float32_and_fail_for_mutants(step, lr, b1, b2, eps):
    """the float32 restatement of k_adam stays inside the three per-element bars; with bias correction 2 omitted, or 1 - b1 used for the
    second moment, it leaves them.  At step 30001 bias correction 2 is 1 to 9e-14 at beta2 = 0.999: omitting it changes nothing there."""
    for n in (5, 1025):
        p, g, m, v = R.adam_inputs(n, 100 + step, moments=step > 10)
        ref = R.adam_ref(p, g, m, v, lr, b1, b2, eps, step)
        shares = R.adam_shares(R.adam_f32(p, g, m, v, lr, b1, b2, eps, step), p, ref, lr, b1, step)
        assert max(shares.values()) <= 1.0, shares
        for mutate in ("no_bc2", "b1_for_v"):
            bad = R.adam_shares(R.adam_f32(p, g, m, v, lr, b1, b2, eps, step, mutate), p, ref, lr, b1, step)
            if mutate == "no_bc2" and step == 30001:
                continue
            assert max(bad.values()) > 1.0, (mutate, n, bad)
            assert bad["exp_avg"] == shares["exp_avg"]


def test_adam_untouched_elements_keep_their_bits_in_the_reference():
    p, g, m, v = R.adam_inputs(64, 1, moments=True)
    still = (g == 0) & (m == 0) & (v == 0)
    assert still.sum() == 4 and ((g == 0) & (m != 0)).sum() == 4
    p64 = R.adam_ref(p, g, m, v, 1.6e-4, 0.9, 0.999, 1e-15, 30001)[0]
    assert np.array_equal(p64[still], p[still].astype(np.float64))


def test_depth_l1_ref():
    pred = np.array([[[1.0, 2.0, 1000.0, np.inf], [3.0, np.nan, 4.0, 5.0]]], np.float32)
    tgt = np.array([[[2.0, 2.0, 1.0, 1.0], [1000.0, 1.0, 1.0, 7.0]]], np.float32)
    with np.errstate(invalid="ignore"):
        valid, diff, cnt, want = R.depth_l1_ref(pred, tgt)
    assert valid.tolist() == [[[True, True, False, False], [False, False, True, True]]]
    assert cnt.tolist() == [4] and want.tolist() == [(1.0 + 0.0 + 3.0 + 2.0) / 4] and diff[0, 1].tolist() == [0.0, 0.0, 3.0, -2.0]
