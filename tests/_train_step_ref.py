"""References and bars of the training-step kernels (gaussctrl_amd/csrc/train_step.hip): fused L1+SSIM, depth L1, fused Adam.

Plain torch / numpy on the CPU, float64-capable; a helper like _margins.py.  tests/test_train_step_ref_cpu.py holds it to oracle/sd15_torch.py
and torch.optim.Adam and shows that every bar below can fail; tests/test_train_step_gpu.py holds the kernels to it.

  ssim_map / splat_loss_ref   the SSIM formula of oracle/sd15_torch.py::ssim as a per-pixel map, and (1-l) L1 + l (1 - mean SSIM) with its
                              gradient by autograd, in float64 (the reference) or float32 (the yardstick of what float32 allows)
  make_images                 the four kinds of image pair the kernels are held on
  ssim_case                   one (image pair, window mode, lambda): float64 loss and gradient, the float32 oracle's own errors, the bars
  adam_ref / adam_f32         Adam at the float32-rounded hyper-parameters in float64, and its float32 restatement (CPU checks only)
  adam_inputs / adam_shares   tensors that mix gradient magnitude classes element by element; the worst share of each per-element bar
  depth_l1_ref                the float64 depth L1 of tests/test_raster_depth_gpu.py::test_depth_l1_loss
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24                       # unit roundoff of float32
C2 = 0.03 ** 2
KINDS = ("uniform", "residual", "flat", "equal")
PADDED_ONLY = ((1, 1), (5, 7))                                       # smaller than the 11 x 11 window
BOTH_MODES = ((11, 11), (12, 40), (16, 16), (17, 33), (44, 37))      # one SSIM pixel; window + 1; one tile; tile + 1 and two tiles + 1; 3 x 3 tiles
CHANNELS = (1, 3, 4)


def modes_of(H, W):
    return (False,) if (H, W) in PADDED_ONLY else (True, False)


# ------------------------------------------------------------------------------------------------------------------------ L1 + SSIM
def ssim_map(a, b, valid=True, dtype=torch.float64, sigma=1.5, c2=0.03 ** 2):
    """oracle/sd15_torch.py::ssim(a, b, valid=valid) before its mean: [B,C,H,W] -> [B,C,H',W'] (the same operations in the same order, so
    the mean has the oracle's bits).  sigma / c2 differ from the defaults only in the mutation checks."""
    a, b = a.to(dtype), b.to(dtype)
    window = 11
    coords = torch.arange(window, dtype=a.dtype, device=a.device) - window // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2)); g = (g / g.sum())
    k = (g[:, None] * g[None, :])[None, None].expand(a.shape[1], 1, window, window)
    mu = lambda x: F.conv2d(x, k, padding=0 if valid else window // 2, groups=x.shape[1])
    ma, mb = mu(a), mu(b)
    va, vb, cab = mu(a * a) - ma * ma, mu(b * b) - mb * mb, mu(a * b) - ma * mb
    c1 = 0.01 ** 2
    return ((2 * ma * mb + c1) * (2 * cab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))


def splat_loss_ref(pred, tgt, lam, valid, dtype=torch.float64, sigma=1.5, c2=0.03 ** 2):
    """oracle/sd15_torch.py::splat_loss on [H,W,C] images in `dtype` -> (loss, d loss / d pred, SSIM map), all in `dtype`"""
    p = pred.detach().to(dtype).clone().requires_grad_(True)
    t = tgt.detach().to(dtype)
    smap = ssim_map(t.permute(2, 0, 1)[None], p.permute(2, 0, 1)[None], valid, dtype, sigma, c2)
    loss = (1 - lam) * (t - p).abs().mean() + lam * (1 - smap.mean())
    (grad,) = torch.autograd.grad(loss, p)
    return loss.detach(), grad, smap.detach()


def _smooth(H, W, C, g):
    """products of low-frequency sines per channel, in [0.1, 0.9]"""
    y = torch.arange(H, dtype=torch.float64)[:, None, None] / max(H, 2)
    x = torch.arange(W, dtype=torch.float64)[None, :, None] / max(W, 2)
    fy = 0.6 + 0.9 * torch.rand(C, generator=g, dtype=torch.float64); fx = 0.6 + 0.9 * torch.rand(C, generator=g, dtype=torch.float64)
    py, px = torch.rand(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64)
    return (0.5 + 0.4 * torch.sin(2 * np.pi * (fy * y + py)) * torch.sin(2 * np.pi * (fx * x + px))).float()


def make_images(kind, H, W, C, seed):
    """-> (pred, target), float32 [H,W,C] in [0, 1]
    uniform   two torch.rand images (what the first tests used)
    residual  a smooth target, pred = target + 0.01 randn, clamped: a render close to its target
    flat      the same with the top half of the target 0.0 and its left third 1.0 (flat backgrounds), and the top quarter of pred
              equal to the target (exact ties inside a flat region)
    equal     pred is a copy of the smooth target"""
    g = torch.Generator().manual_seed(int(seed))
    if kind == "uniform":
        return torch.rand(H, W, C, generator=g), torch.rand(H, W, C, generator=g)
    tgt = _smooth(H, W, C, g)
    if kind == "equal":
        return tgt.clone(), tgt
    if kind == "flat":
        tgt[:H // 2] = 0.0
        tgt[:, :W // 3] = 1.0
    pred = (tgt + 0.01 * torch.randn(H, W, C, generator=g)).clamp(0.0, 1.0)
    if kind == "flat":
        pred[:H // 4] = tgt[:H // 4]
    elif kind != "residual":
        raise ValueError(kind)
    return pred, tgt


def grad_measure(grad, grad64):
    """max |grad - grad64| * n: the error in units of the L1 gradient's size 1 / n (never zero, unlike max |grad64| on `equal` images)"""
    return float((grad.detach().cpu().double() - grad64).abs().max()) * grad64.numel()


def grad_bar(kind, lam, n, n_ssim, e32):
    """equal: three window sums of partials as large as 1 / C2 cancel, 16 roundings of their size may remain;
    otherwise 4 x the float32 oracle's own error (two bits for another association of the same ill-conditioned expression), and no less
    than 16 roundings (about 44 window taps of float32 accumulation)"""
    if kind == "equal":
        return 16 * U * lam / C2 * n / n_ssim
    return max(4 * e32, 16 * U)


@functools.lru_cache(maxsize=None)
def ssim_case(kind, H, W, C, valid, lam=0.2):
    """the reference of one case, computed once: inputs, float64 loss / gradient, and the bars from the float32 oracle on the same inputs"""
    pred, tgt = make_images(kind, H, W, C, seed=1000 * H + 10 * W + C)
    loss64, grad64, map64 = splat_loss_ref(pred, tgt, lam, valid, torch.float64)
    _, grad32, map32 = splat_loss_ref(pred, tgt, lam, valid, torch.float32)
    n = H * W * C
    n_ssim = (H - 10) * (W - 10) * C if valid else n
    assert map64.numel() == n_ssim
    e32 = grad_measure(grad32, grad64)
    return dict(pred=pred, tgt=tgt, loss64=float(loss64), grad64=grad64, n=n, n_ssim=n_ssim, e32=e32,
                grad_bar=grad_bar(kind, lam, n, n_ssim, e32),
                loss_bar=lam * 4 * float((map32.double() - map64).abs().mean()) + 4 * U * max(1.0, abs(float(loss64))))


# ------------------------------------------------------------------------------------------------------------------------------- Adam
GRAD_CLASSES = (0.0, 1e-20, 1e-17, 1e-12, 1e-6, 1.0, 1e4, 1e18)


def adam_inputs(n, seed, moments):
    """float32 (p, g, m, v) of n elements; element i has gradient size GRAD_CLASSES[i % 8] (exactly 0, of either sign, in class 0).
    moments=False: zero moments (a first step); True: moments of the gradient's size (a resumed checkpoint) -- in class 0 every other octet
    keeps zero moments (a row no view ever touched) and the rest decays moments of size 1e-3."""
    r = np.random.default_rng(seed)
    cls = np.asarray(GRAD_CLASSES)[np.arange(n) % 8]
    p = r.standard_normal(n).astype(np.float32)
    g = (cls * r.uniform(0.5, 1.5, n) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    if not moments:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    size = np.where((cls == 0.0) & ((np.arange(n) // 8) % 2 == 1), 1e-3, cls)
    m = (size * 0.3 * r.standard_normal(n) + 0.0).astype(np.float32)              # (+ 0.0: zero moments are +0, as zeros_like leaves them)
    v = (size * size * r.uniform(0.5, 1.5, n)).astype(np.float32)
    return p, g, m, v


def adam_ref(p, g, m, v, lr, b1, b2, eps, step):
    """One torch.optim.Adam step in float64 at the float32-rounded hyper-parameters (what the C ABI receives), both bias corrections formed
    in double from the rounded values as gc_adam_step's host code does -> (p, m, v, mag, den):
    mag = |b1 m| + |(1 - b1) g| (the operands of the first moment), den = sqrt(v_new) / sqrt(bc2) + eps."""
    lr, b1, b2, eps = (float(np.float32(x)) for x in (lr, b1, b2, eps))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    mag = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    den = np.sqrt(v) / np.sqrt(bc2) + eps
    return p - (lr / bc1) * m / den, m, v, mag, den


def adam_f32(p, g, m, v, lr, b1, b2, eps, step, mutate=None):
    """k_adam's expressions in float32 numpy (every operation rounded, no contraction) -> (p, m, v).
    mutate: "no_bc2" omits bias correction 2, "b1_for_v" uses 1 - b1 for the second moment."""
    f = np.float32
    lr, b1, b2, eps = f(lr), f(b1), f(b2), f(eps)
    bc1, bc2 = 1.0 - float(b1) ** step, 1.0 - float(b2) ** step
    step_size, inv_sqrt_bc2 = f(float(lr) / bc1), f(1.0 if mutate == "no_bc2" else 1.0 / np.sqrt(bc2))
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    with np.errstate(under="ignore"):
        m = b1 * m + (f(1) - b1) * g
        v = b2 * v + (f(1) - (b1 if mutate == "b1_for_v" else b2)) * g * g
        p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
    return p, m, v


def ulp32(x):
    """spacing of float32 at |x| (x in float64)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def adam_shares(got, p_old, ref, lr, b1, step):
    """worst share of the per-element bars used by got = (p, m, v) against ref = adam_ref(...) -> {"param", "exp_avg", "exp_avg_sq"}:
      |m - m64| <= 3 U mag + 1.4e-45
      |v - v64| <= 3 ulp(v64)                    all terms positive: two products, a square, one sum
      |p - p64| <= 0.5 max(ulp(p_old), ulp(p64)) + 8 U lr_hat mag / den,   lr_hat = float32(lr) / bc1
    mag and not |m64|: an element whose b1 m and (1 - b1) g cancel is judged by its operands."""
    p64, m64, v64, mag, den = ref
    lr_hat = float(np.float32(lr)) / (1.0 - float(np.float32(b1)) ** step)
    gp, gm, gv = (np.asarray(a, np.float64) for a in got)
    bars = {"param": 0.5 * np.maximum(ulp32(p_old), ulp32(p64)) + 8 * U * lr_hat * mag / den,
            "exp_avg": 3 * U * mag + 1.4e-45,
            "exp_avg_sq": 3 * ulp32(v64)}
    errs = {"param": np.abs(gp - p64), "exp_avg": np.abs(gm - m64), "exp_avg_sq": np.abs(gv - v64)}
    return {k: float((errs[k] / bars[k]).max()) for k in bars}


# --------------------------------------------------------------------------------------------------------------------------- depth L1
def depth_l1_ref(pred, target):
    """[B,H,W] float32 depth images -> (valid mask, pred - target on the valid pixels and 0 elsewhere, valid count per view, loss per view),
    in float64: a pixel is valid when neither depth is the 1000 of an empty pixel and both are finite"""
    B = pred.shape[0]
    pd, td = pred.astype(np.float64), target.astype(np.float64)
    valid = (pd != 1000.0) & (td != 1000.0) & np.isfinite(pd) & np.isfinite(td)
    diff = np.where(valid, pd - np.where(valid, td, 0.0), 0.0)
    cnt = valid.reshape(B, -1).sum(1)
    want = np.abs(diff).reshape(B, -1).sum(1) / np.maximum(cnt, 1)
    return valid, diff, cnt, want
