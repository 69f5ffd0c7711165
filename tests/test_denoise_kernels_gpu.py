"""GPU parity of the individual denoise kernels (through the C ABI) against plain PyTorch fp32/fp64
references of the same op evaluated on the SAME 2-byte-rounded inputs.  Tolerance: one output rounding of
the activation dtype (bf16: 2^-8, f16: 2^-11 relative) plus accumulation-order noise."""
import dataclasses

import numpy as np
import pytest
from _margins import within
from _redzone import on_device
import torch
import torch.nn.functional as F

from gaussctrl_amd.sd.ops import GC_GEMM_VAR_NO_LEAN_LN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTS = [torch.bfloat16, torch.float16]
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def _close(got, ref, dt, extra=1.0):
    """|err| <= tol * |ref| (ONE output rounding of the activation dtype: deterministic, can be used up entirely at the bottom of a
    binade) + 0.05 * tol * max|ref| + 1e-6 (slack for accumulation-order noise).  The recorded margin is the share of that SLACK in use."""
    got = got.double().cpu(); ref = ref.double().cpu()
    tol = EPS[dt] * extra
    err = (got - ref).abs()
    slack = tol * ref.abs().max() * 0.05 + 1e-6
    within("kernel output: (err - one rounding) / accumulation slack", ((err - tol * ref.abs()) / slack).clamp_min(0).max().item(), 1.0)


def _rand(shape, dt, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    v = (torch.randn(shape, generator=g) * scale).to(dt)
    out = torch.empty(v.shape, dtype=dt, device=DEV)          # (a torch factory, not .to(DEV): under the red-zone guard the input is carved too)
    out.copy_(v)
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 320, 320), (1000, 640, 2560), (77 * 2, 320, 768), (14, 1280, 320), (4096, 1280, 1280)])
def test_linear(dt, M, N, K):
    from gaussctrl_amd.sd import ops
    x = _rand((M, K), dt, 1.0, 1); w = _rand((N, K), dt, K ** -0.5, 2)
    b = torch.randn(N, device=DEV); r = _rand((M, N), dt, 1.0, 3)
    ref = x.double() @ w.double().T + b.double()
    _close(ops.linear(x, w, b), ref, dt)
    _close(ops.linear(x, w, b, out_f32=True), ref, dt, extra=0.05)
    _close(ops.linear(x, w, b, residual=r), ref + r.double(), dt)
    _close(ops.linear(x, w, b, act=1, scale=0.5), F.silu(ref) * 0.5, dt)


@pytest.mark.parametrize("dt", DTS)
def test_linear_geglu_rowvec_transposed(dt):
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import geglu_permute
    M, K, C4 = 512, 320, 1280
    x = _rand((M, K), dt, 1.0, 1); w = _rand((2 * C4, K), dt, K ** -0.5, 2); b = torch.randn(2 * C4, device=DEV)
    pr = x.double() @ w.double().T + b.double()
    hid, gate = pr.chunk(2, dim=-1)
    ref = hid * F.gelu(gate)
    wp, bp = geglu_permute(w, b)
    _close(ops.linear(x, wp, bp, geglu=True), ref, dt, extra=2.0)
    # rowvec (time-embedding add) + transposed copy (V operand)
    Bn, Lt, N = 4, 128, 320
    x = _rand((Bn, Lt, K), dt, 1.0, 4); w = _rand((N, K), dt, K ** -0.5, 5)
    rv = torch.randn(Bn, N, device=DEV)
    ref = x.double() @ w.double().T + rv.double()[:, None, :]
    vt = torch.zeros(Bn, N, Lt + 8, dtype=dt, device=DEV)
    out = ops.linear(x, w, None, rowvec=rv, rows_per_batch=Lt, out_t=vt, ldt=Lt + 8, t_batch_stride=N * (Lt + 8))
    _close(out, ref, dt)
    _close(vt[:, :, :Lt], ref.transpose(1, 2), dt)
    assert float(vt[:, :, Lt:].abs().max()) == 0.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,K,N,geglu", [(24576, 320, 2560, True), (6144, 640, 5120, True), (24576 + 77, 320, 2560 + 128, False),
                                         (70000, 64, 640, False)])
def test_linear_persistent_multi_round(dt, M, K, N, geglu):
    """Multi-round short-K linears take the persistent kernel (k_gemm8p: > 256 tiles of 256 x 128, next tile's fill under the
    epilogue): GEGLU FF-up shapes of the 64x64 / 32x32 levels, a ragged M / N case and a one-k-tile case; bias, SiLU + scale, residual."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import geglu_permute
    x = _rand((M, K), dt, 1.0, 1); w = _rand((N, K), dt, K ** -0.5, 2); b = torch.randn(N, device=DEV)
    pr = x.double() @ w.double().T + b.double()
    if geglu:
        hid, gate = pr.chunk(2, dim=-1)
        wp, bp = geglu_permute(w, b)
        _close(ops.linear(x, wp, bp, geglu=True), hid * F.gelu(gate), dt, extra=2.0)
    else:
        r = _rand((M, N), dt, 1.0, 3)
        _close(ops.linear(x, w, b), pr, dt)
        _close(ops.linear(x, w, b, residual=r), pr + r.double(), dt)
        _close(ops.linear(x, w, b, act=1, scale=0.5), F.silu(pr) * 0.5, dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride,ups", [(2, 16, 16, 64, 128, 1, False), (3, 16, 12, 320, 320, 1, False),
                                                       (2, 16, 16, 128, 64, 2, False), (2, 8, 8, 64, 64, 1, True),
                                                       (2, 32, 32, 8, 320, 1, False), (1, 64, 64, 16, 32, 2, False),
                                                       (2, 9, 7, 96, 96, 2, False), (14, 8, 8, 2560, 1280, 1, False)])
def test_conv3x3(dt, B, H, W, Cin, Cout, stride, ups):
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight
    x = _rand((B, H, W, Cin), dt, 1.0, 1)
    w = _rand((Cout, Cin, 3, 3), dt, (9 * Cin) ** -0.5, 2)
    b = torch.randn(Cout, device=DEV)
    xin = x.double().permute(0, 3, 1, 2)
    if ups:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.double(), b.double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    wp = conv3x3_weight(w, dt)
    _close(ops.conv3x3(x, wp, b, stride=stride, upsample=ups), ref, dt)
    rv = torch.randn(B, Cout, device=DEV); res = _rand(tuple(ref.shape), dt, 1.0, 3)
    got = ops.conv3x3(x, wp, b, stride=stride, upsample=ups, rowvec=rv, residual=res)
    _close(got, ref + rv.double()[:, None, None, :] + res.double(), dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,HW,C,G", [(2, 256, 320, 32), (3, 64, 1280, 32), (2, 100, 2560, 32), (2, 1024, 128, 32), (1, 4, 1920, 32), (2, 36, 960, 32)])
def test_groupnorm(dt, B, HW, C, G):
    from gaussctrl_amd.sd import ops
    x = (_rand((B, HW, C), dt, 1.0, 1).float() * 2 + 3.0).to(dt)        # |mean| > std: exercises the shifted sums
    gamma = torch.randn(C, device=DEV); beta = torch.randn(C, device=DEV)
    ref = F.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), 1e-5).transpose(1, 2)
    _close(ops.groupnorm(x, gamma, beta, G, 1e-5, False), ref, dt, extra=2.0)
    _close(ops.groupnorm(x, gamma, beta, G, 1e-5, True), F.silu(ref), dt, extra=2.0)


def _parts_sums(parts, b, HW, cpg):
    """add up the slabs / halves of batch b the way gc_dn_groupnorm_apply_parts does -> [G, 2]"""
    if parts.mode == 1:
        ns = (HW + parts.rows - 1) // parts.rows
    else:
        ns = ((b + 1) * HW - 1) // parts.rows - (b * HW) // parts.rows + 1
    assert ns <= parts.nslab
    p = parts.buf[b, :ns].double()                      # [ns, G, 2 halves, 2]
    tot = p[:, :, 0].sum(0)
    for g in range(parts.groups):                       # half 1 is defined only for a group that straddles two column tiles
        if (g * cpg) // parts.col_tile != ((g + 1) * cpg - 1) // parts.col_tile:
            tot[g] += p[:, g, 1].sum(0)
    return tot


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,B,H,Cin,Cout", [("conv", 6, 64, 320, 320),        # MT 3 tiles of 192 rows straddle the 4096-row batches
                                               ("conv", 2, 32, 320, 640), ("conv", 6, 32, 640, 640), ("conv", 3, 64, 640, 320),
                                               ("conv", 6, 16, 1280, 1280),      # split-K: the reduce-epilogue kernel leaves the partials
                                               ("conv", 2, 16, 640, 1280), ("conv_in", 6, 64, 8, 320), ("down", 6, 64, 320, 320),
                                               ("linear", 6, 32, 640, 640), ("linear", 6, 16, 1280, 1280), ("linear", 2, 64, 320, 320),
                                               ("concat", 6, 64, 320, 320), ("concat", 6, 32, 640, 320), ("concat", 2, 16, 1280, 640),
                                               ("concat", 2, 18, 320, 320)])     # HW 324: 3 pixel lanes, a last slab of 4 pixels
def test_groupnorm_from_producer_partials(dt, kind, B, H, Cin, Cout):
    """The statistics pass of a GroupNorm as per-channel partial sums left by the kernel that PRODUCED the tensor (conv / linear epilogue,
    split-K reduce, concat): the partials add up to the channel sums of the stored output, and GroupNorm(+SiLU) from them equals the
    stand-alone three-kernel GroupNorm and the fp64 reference (inputs with |mean| > std: raw fp32 sums must not cancel visibly)."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight
    G = 32
    if kind in ("conv", "conv_in", "down"):
        x = _rand((B, H, H, Cin), dt, 1.0, 1)
        w = _rand((Cout, Cin, 3, 3), dt, (9 * Cin) ** -0.5, 2)
        b = torch.randn(Cout, device=DEV) * 2 + 1.5
        res = _rand((B, H, H, Cout), dt, 1.0, 3) if kind == "conv" else None
        out, parts = ops.conv3x3(x, conv3x3_weight(w, dt), b, stride=2 if kind == "down" else 1, residual=res, chan_parts=True)
        plain = ops.conv3x3(x, conv3x3_weight(w, dt), b, stride=2 if kind == "down" else 1, residual=res)
    elif kind == "linear":
        x = _rand((B, H * H, Cin), dt, 1.0, 1)
        w = _rand((Cout, Cin), dt, Cin ** -0.5, 2)
        b = torch.randn(Cout, device=DEV) * 2 + 1.5
        res = _rand((B, H * H, Cout), dt, 1.0, 3)
        out, parts = ops.linear(x, w, b, residual=res, rows_per_batch=H * H, chan_parts=True)
        plain = ops.linear(x, w, b, residual=res, rows_per_batch=H * H)
    else:
        a = (_rand((B, H, H, Cin), dt, 1.0, 1).float() + 2.0).to(dt); bb = _rand((B, H, H, Cout), dt, 1.0, 2); cc = _rand((B, H, H, Cout), dt, 1.0, 3)
        out, parts = ops.concat_add(a, bb, cc, chan_parts=True)
        plain = ops.concat_add(a, bb, cc)
    if parts is None and ops.OPTIONS.gemm_variant:
        pytest.skip("a forced kernel variant (tests/test_gemm_variants_gpu.py) without the statistics epilogue")
    assert parts is not None, "this shape must take the producer-statistics path"
    assert torch.equal(out, plain)                          # the statistics epilogue does not change what is stored
    Bo, Co = out.shape[0], out.shape[-1]
    HW = out.numel() // (Bo * Co)
    o64 = out.double().reshape(Bo, HW, Co)
    cpg = Co // G
    for bi in range(Bo):
        got = _parts_sums(parts, bi, HW, cpg)
        og = o64[bi].reshape(HW, G, cpg)
        want = torch.stack([og.sum((0, 2)), (og ** 2).sum((0, 2))], -1)
        within(f"{kind}: group partial sums vs fp64 (rel to sum |x| resp. sum x^2)",
               ((got - want).abs() / torch.stack([og.abs().sum((0, 2)), (og ** 2).sum((0, 2))], -1).clamp_min(1e-6)).max().item(), 2e-6)
    gamma = torch.randn(Co, device=DEV); beta = torch.randn(Co, device=DEV)
    ref = F.group_norm(o64.transpose(1, 2), G, gamma.double(), beta.double(), 1e-5).transpose(1, 2).reshape(out.shape)
    for silu in (False, True):
        y = ops.groupnorm(out, gamma, beta, G, 1e-5, silu, parts=parts)
        _close(y, F.silu(ref) if silu else ref, dt, extra=2.0)
        y3 = ops.groupnorm(out, gamma, beta, G, 1e-5, silu)
        within(f"{kind}: GroupNorm from partials vs the stand-alone kernels (max abs diff / max |y|)",
               ((y.double() - y3.double()).abs().max() / y3.double().abs().max()).item(), 2 * EPS[dt])
    coef = ops.groupnorm_coef(out.reshape(Bo, HW, Co), gamma, beta, G, 1e-5, parts=parts)
    coef3 = ops.groupnorm_coef(out.reshape(Bo, HW, Co), gamma, beta, G, 1e-5)
    within(f"{kind}: coefficients from partials vs stand-alone", ((coef - coef3).abs().max() / coef3.abs().max()).item(), 1e-4)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,C", [(100, 320), (77, 640), (1000, 1280), (5, 64)])
def test_layernorm(dt, M, C):
    from gaussctrl_amd.sd import ops
    x = _rand((M, C), dt, 2.0, 1)
    gamma = torch.randn(C, device=DEV); beta = torch.randn(C, device=DEV)
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    _close(ops.layernorm(x, gamma, beta), ref, dt, extra=2.0)


def _ref_attn(q, k, v, heads, scale):
    B, Lq, C = q.shape
    D = C // heads
    qh = q.double().reshape(B, Lq, heads, D).permute(0, 2, 1, 3)
    kh = k.double().reshape(k.shape[0], k.shape[1], heads, D).permute(0, 2, 1, 3)
    vh = v.double().reshape(v.shape[0], v.shape[1], heads, D).permute(0, 2, 1, 3)
    o = ((qh @ kh.transpose(-1, -2)) * scale).softmax(-1) @ vh
    return o.permute(0, 2, 1, 3).reshape(B, Lq, C)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f,L,heads,D,coeff", [(5, 256, 8, 40, 0.6), (7, 100, 8, 80, 0.6), (5, 64, 8, 160, 0.0), (6, 4, 8, 160, 0.6),
                                               (5, 256, 8, 160, 0.6), (4, 256, 8, 160, 0.0), (4, 128, 8, 160, 0.0), (5, 64, 8, 160, 0.6), (4, 192, 8, 160, 0.6),
                                               (5, 1024, 2, 40, 0.6), (5, 70, 2, 8, 0.6), (5, 200, 3, 40, 0.6), (5, 64, 2, 40, 0.0),
                                               (5, 136, 2, 80, 0.6)])
def test_cross_view_attention(dt, f, L, heads, D, coeff):
    """a*self + (1-a)*mean of the 4 reference attentions (utils.py:86-117) in one fused kernel."""
    from gaussctrl_amd.sd import ops
    B, C = 2 * f, heads * D
    q = _rand((B, L, C), dt, 1.0, 1); k = _rand((B, L, C), dt, 1.0, 2); v = _rand((B, L, C), dt, 1.0, 3)
    Lp = (L + 7) // 8 * 8
    vt = torch.zeros(B, C, Lp, dtype=dt, device=DEV); vt[:, :, :L] = v.transpose(1, 2)
    scale = D ** -0.5
    ref = coeff * _ref_attn(q, k, v, heads, scale)
    for r in range(4):
        idx = torch.arange(B, device=DEV) // f * f + r
        ref = ref + (1 - coeff) / 4 * _ref_attn(q, k[idx], v[idx], heads, scale)
    sets = ([(-1, coeff)] if coeff != 0 else []) + [(r, (1 - coeff) / 4) for r in range(4)]
    got = ops.attention(q, k, vt, heads, sets, f, Lk=L)
    _close(got, ref, dt, extra=8.0)      # P is rounded to the activation dtype before P V (as in the reference's fp16 bmm)
    # the same through a separate reference bank (cached reference K/V)
    bank_idx = on_device(torch.cat([torch.arange(4), f + torch.arange(4)]), DEV)
    got2 = ops.attention(q, k, vt, heads, sets, f, Lk=L, kref=k[bank_idx].contiguous(), vtref=vt[bank_idx].contiguous(), ref_fph=4)
    assert torch.equal(got, got2)
    # product path: softmax scale * log2(e) already folded into Q (weights.prepare(heads=...)): P = exp2(q'.k)
    qp = (q.float() * (scale * 1.4426950408889634)).to(dt)
    refp = coeff * _ref_attn(qp, k, v, heads, float(np.log(2.0)))
    for r in range(4):
        idx = torch.arange(B, device=DEV) // f * f + r
        refp = refp + (1 - coeff) / 4 * _ref_attn(qp, k[idx], v[idx], heads, float(np.log(2.0)))
    _close(ops.attention(qp, k, vt, heads, sets, f, Lk=L, q_prescaled=True), refp, dt, extra=8.0)


@pytest.mark.parametrize("dt", DTS)
def test_text_attention_and_rescale_branch(dt):
    """plain attention against 77 shared text keys (kind -2) + a spiked key that forces the online-softmax rescale."""
    from gaussctrl_amd.sd import ops
    f, L, heads, D, Lt = 3, 200, 8, 40, 77
    B, C = 2 * f, heads * D
    q = _rand((B, L, C), dt, 1.0, 1); k = _rand((2, Lt, C), dt, 1.0, 2); v = _rand((2, Lt, C), dt, 1.0, 3)
    k[:, 70, :] = k[:, 70, :] * 6.0          # lands in the 2nd key tile: max jumps after the first tile
    vt = torch.zeros(2, C, 80, dtype=dt, device=DEV); vt[:, :, :Lt] = v.transpose(1, 2)
    idx = torch.arange(B, device=DEV) // f
    ref = _ref_attn(q, k[idx], v[idx], heads, D ** -0.5)
    got = ops.attention(q, k, vt, heads, [(-2, 1.0)], f, Lk=Lt)
    _close(got, ref, dt, extra=8.0)


@pytest.mark.parametrize("dt", DTS)
def test_attention_offset_overflow_falls_back(dt):
    """The fast kernel keeps the first key tile's row maximum as a fixed softmax offset; a later key that beats it by far more
    than the exponent range must trigger the in-kernel safe recomputation (same answer as the online-softmax kernel)."""
    from gaussctrl_amd.sd import ops
    f, L, heads, D = 2, 256, 2, 40
    B, C = 2 * f, heads * D
    q = _rand((B, L, C), dt, 1.0, 1); k = _rand((B, L, C), dt, 1.0, 2); v = _rand((B, L, C), dt, 1.0, 3)
    k[:, 200, :] = q[:, 17, :] * 40.0         # logit of (query 17, key 200) ~ 40 * |q|^2 / sqrt(D) ~ 250 >> first-tile maximum
    vt = v.transpose(1, 2).contiguous()
    ref = _ref_attn(q, k, v, heads, D ** -0.5)
    got = ops.attention(q, k, vt, heads, [(-1, 1.0)], f, Lk=L)
    assert torch.isfinite(got.float()).all()
    _close(got, ref, dt, extra=8.0)


@pytest.mark.parametrize("dt", DTS)
def test_elementwise_and_ddim(dt):
    from gaussctrl_amd.sd import ops
    a = _rand((4, 10, 10, 64), dt, 1.0, 1); b = _rand((4, 10, 10, 32), dt, 1.0, 2); c = _rand((4, 10, 10, 32), dt, 1.0, 3)
    _close(ops.concat_add(a, b, c), torch.cat([a.double(), b.double() + c.double()], -1), dt)
    assert torch.equal(ops.concat_add(a, b), torch.cat([a, b], -1))
    _close(ops.axpby(b, 0.5, c, 2.0, act=1), F.silu(0.5 * b.double() + 2.0 * c.double()), dt)
    x = torch.randn(7, 1280, device=DEV)
    _close(ops.cast_f32(x, dt, silu=True), F.silu(x.double()), dt)
    s = _rand((37, 300), dt, 3.0, 4); ref = (s.double() * 0.3).softmax(-1)
    _close(ops.softmax_rows_(s.clone(), 0.3), ref, dt, extra=2.0)
    f, H, W = 3, 8, 8
    eps = torch.randn(2 * f, H, W, 8, device=DEV); lat = torch.randn(f, H, W, 4, device=DEV)
    xin = torch.full((2 * f, H, W, 8), 7.0, dtype=dt, device=DEV)
    a_t, a_p, gs = 0.3, 0.45, 5.0
    e = eps[:f, ..., :4] + gs * (eps[f:, ..., :4] - eps[:f, ..., :4])
    x0 = (lat - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
    want = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * e
    ops.cfg_ddim_step(eps, lat, xin, gs, True, a_t, a_p, 2)
    assert torch.allclose(lat, want, atol=2e-5)
    _close(xin[:f, ..., :4], want, dt); assert torch.equal(xin[:f], xin[f:]); assert float(xin[..., 4:].abs().max()) == 0


# ------------------------------------------------------------------------------------------- fused normalisation (round 2)
def _sums(t):
    t = t.double()
    return torch.stack([t.sum(-1), (t * t).sum(-1)], -1)


def _group_sums(out_bln, G):
    """[B, L, N] -> [B, G, 2] (sum, sum^2) over the L rows and the N / G channels of each group"""
    B, L, N = out_bln.shape
    return _sums(out_bln.double().reshape(B, L, G, N // G).permute(0, 2, 1, 3).reshape(B, G, -1))


def _sums_abs(t):
    """the scale of _sums' two columns: (sum |x|, sum x^2) -- what fp32 accumulation noise is relative to"""
    t = t.double()
    return torch.stack([t.abs().sum(-1), (t * t).sum(-1)], -1)


def _group_sums_abs(out_bln, G):
    B, L, N = out_bln.shape
    return _sums_abs(out_bln.double().reshape(B, L, G, N // G).permute(0, 2, 1, 3).reshape(B, G, -1))


def _stats_close(got, ref, scale):
    """(sum, sum^2) partials accumulated in fp32 by the kernel (lane sums, DPP / LDS reduction, atomics in arbitrary order) against the fp64 sums of the stored
    output: |err| <= 2e-6 x (sum |x|, sum x^2) -- ~30 fp32 ulps of what was added up, the bar of test_groupnorm_from_producer_partials -- or the original bar.  Round 6: the bar was ONLY
    2e-5 relative to the SIGNED sum (+ 1e-3 of the largest entry); a group whose sum happens to be near zero then has an absolute allowance of a few 1e-4 on ten
    thousand fp32 additions of O(1) values, and with bias / row vector drawn from the (per-process random) CUDA generator 1-7 draws in 2 000 exceeded it
    (scripts/diag/group_stats_margin.py: errors of 1.2e-3 on sum |x| = 1.6e4, i.e. 7.5e-8 = 1.3 ulp) -- the intermittent failure of the forced-tile children."""
    got = got.double().cpu(); ref = ref.cpu(); scale = scale.cpu().clamp_min(1e-6)
    err = (got - ref).abs()
    # an entry passes on EITHER form, each normalised to 1: the original relative bar (2e-5 of |ref| + 1e-3 max|ref|) or the accumulation-noise floor (2e-6 of the
    # entry's scale); the noise floor is what the near-zero sums need, the relative one what the large all-positive sums were always held to
    used = torch.minimum(err / (2e-5 * (ref.abs() + 1e-3 * ref.abs().max())), err / (2e-6 * scale))
    worst = float(used.max())
    if not worst < 1.0:
        idx = tuple((used == used.max()).nonzero()[0].tolist())
        raise AssertionError(f"STATS-MISMATCH x{worst:.3f} of the bar at {idx}: got {float(got[idx]):.9g} want {float(ref[idx]):.9g} scale {float(scale[idx]):.6g}; "
                             f"{int((used >= 1.0).sum())} of {used.numel()} entries off; got finite {bool(torch.isfinite(got).all())}")
    within("statistics partials: |err| / min(2e-5 (|ref| + 1e-3 max|ref|), 2e-6 (sum |x| resp. sum x^2))", worst, 1.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,L,N,K", [(2, 256, 320, 320), (6, 4096, 320, 320), (3, 64, 1280, 1280), (2, 1024, 640, 640), (2, 80, 320, 5120),
                                     (6, 256, 1280, 5120)])
def test_linear_output_statistics(dt, B, L, N, K):
    """producer side: (sum, sum^2) of the STORED output per row (slab partials -> LayerNorm fold) and per (batch, GroupNorm group)
    (-> GroupNorm apply), left by the GEMM epilogue (every k_gemm8 / k_gemm / split-K variant via test_gemm_variants_gpu)."""
    from gaussctrl_amd.sd import ops
    x = _rand((B, L, K), dt, 1.0, 1); w = _rand((N, K), dt, K ** -0.5, 2)
    b = torch.randn(N, device=DEV); r = (_rand((B, L, N), dt, 1.0, 3).float() + 1.5).to(dt)
    rs = ops.RowStats(); gs = torch.zeros(B, 32, 2, device=DEV)
    out = ops.linear(x, w, b, residual=r, rows_per_batch=L, row_stats=rs, group_stats=gs)
    _close(out, x.double() @ w.double().T + b.double() + r.double(), dt)
    assert rs.buf.shape == (rs.slots, B * L, 2) and rs.slots >= 1
    _stats_close(rs.buf.sum(0), _sums(out.view(B * L, N)), _sums_abs(out.view(B * L, N)))
    _stats_close(gs, _group_sums(out, 32), _group_sums_abs(out, 32))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(6, 64, 64, 320, 320, 1), (2, 32, 32, 640, 640, 1), (3, 16, 16, 1280, 1280, 1),
                                                   (2, 32, 32, 320, 320, 2), (14, 8, 8, 1280, 1280, 1), (2, 16, 16, 64, 96, 1)])
def test_conv_output_group_statistics(dt, B, H, W, Cin, Cout, stride):
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight
    x = _rand((B, H, W, Cin), dt, 1.0, 1)
    w = conv3x3_weight(_rand((Cout, Cin, 3, 3), dt, (9 * Cin) ** -0.5, 2), dt)
    b = torch.randn(Cout, device=DEV); rv = torch.randn(B, Cout, device=DEV)
    gs = torch.zeros(B, 32, 2, device=DEV)
    out = ops.conv3x3(x, w, b, stride=stride, rowvec=rv, group_stats=gs)
    _stats_close(gs, _group_sums(out.reshape(B, -1, Cout), 32), _group_sums_abs(out.reshape(B, -1, Cout), 32))


@pytest.mark.parametrize("kind,B,H,Cin,Cout", [("conv", 6, 64, 320, 320), ("conv", 3, 64, 640, 320), ("conv", 6, 16, 1280, 1280), ("down", 6, 64, 320, 320),
                                               ("linear", 6, 32, 640, 640), ("concat", 6, 64, 320, 320), ("concat", 2, 16, 1280, 640), ("ln", 6, 32, 640, 640)])
def test_statistics_buffers_nan_poisoned(kind, B, H, Cin, Cout, monkeypatch):
    """The statistics buffers (ChanParts, RowStats) come from torch.empty and the consumers trust their own recomputation of which slab /
    half-1 / slot entries the producer wrote (advisor finding, round 4).  Here every buffer is NaN-filled BEFORE the producer launch
    (sd.ops.DEBUG_FILL): a consumer that reads one entry the producer does not write -- straddling row tiles (MT = 3 on 4096-row batches), groups
    that straddle column tiles, split-K reduce, concat, the LayerNorm row partials -- returns NaN."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight
    monkeypatch.setattr(ops, "DEBUG_FILL", float("nan"))
    dt = torch.bfloat16
    G = 32
    if kind in ("conv", "down"):
        x = _rand((B, H, H, Cin), dt, 1.0, 1); w = _rand((Cout, Cin, 3, 3), dt, (9 * Cin) ** -0.5, 2); b = torch.randn(Cout, device=DEV)
        out, parts = ops.conv3x3(x, conv3x3_weight(w, dt), b, stride=2 if kind == "down" else 1, chan_parts=True)
    elif kind == "linear":
        x = _rand((B, H * H, Cin), dt, 1.0, 1); w = _rand((Cout, Cin), dt, Cin ** -0.5, 2)
        out, parts = ops.linear(x, w, None, rows_per_batch=H * H, chan_parts=True)
    elif kind == "concat":
        a = _rand((B, H, H, Cin), dt, 1.0, 1); bb = _rand((B, H, H, Cout), dt, 1.0, 2); cc = _rand((B, H, H, Cout), dt, 1.0, 3)
        out, parts = ops.concat_add(a, bb, cc, chan_parts=True)
    else:                                               # LayerNorm fold: producer row partials -> folded consumer
        x0 = _rand((B * H * H, Cin), dt, 1.0, 1); w0 = _rand((Cout, Cin), dt, Cin ** -0.5, 2)
        rs = ops.RowStats()
        x = ops.linear(x0, w0, None, row_stats=rs)
        assert torch.isfinite(rs.buf).all(), "a row-partial slot the layout query announces was not written"
        wf = _rand((Cout, Cout), dt, Cout ** -0.5, 3)
        y = ops.linear(x, wf, torch.zeros(Cout, device=DEV), ln=(rs, wf.float().sum(1).contiguous(), 1e-5))
        assert torch.isfinite(y.float()).all()
        return
    if parts is None and ops.OPTIONS.gemm_variant:
        pytest.skip("forced kernel variant (tests/test_gemm_variants_gpu.py): the 4-wave kernel leaves no channel partials")
    assert parts is not None
    gamma = torch.randn(out.shape[-1], device=DEV); beta = torch.randn(out.shape[-1], device=DEV)
    y = ops.groupnorm(out, gamma, beta, G, 1e-5, True, parts=parts)
    assert torch.isfinite(y.float()).all(), "GroupNorm from the producer's partials read an entry nobody wrote"
    monkeypatch.setattr(ops, "DEBUG_FILL", None)
    y3 = ops.groupnorm(out, gamma, beta, G, 1e-5, True)
    within(f"{kind}: poisoned-buffer GroupNorm vs the stand-alone kernels", ((y.double() - y3.double()).abs().max() / y3.double().abs().max()).item(), 2 * EPS[dt])
    # ... and an inf in ONE batch's rows stays in that batch: a row tile that straddles two batches must not leak it through 0 * inf
    if kind == "conv" and B >= 2 and H == 64:
        x2 = x.clone(); x2[1] = float("inf")
        out2, parts2 = ops.conv3x3(x2, conv3x3_weight(w, dt), b, chan_parts=True)
        y2 = ops.groupnorm(out2, gamma, beta, G, 1e-5, True, parts=parts2)
        assert torch.isfinite(y2[0].float()).all() and torch.isfinite(y2[2:].float()).all(), "another batch's inf leaked through a straddling tile"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", [0, GC_GEMM_VAR_NO_LEAN_LN])
@pytest.mark.parametrize("M,N,K,geglu", [(512, 960, 320, False), (24576, 960, 320, False), (300, 1280, 1280, False), (1024, 2560, 320, True),
                                         (384, 10240, 1280, True), (6144, 5120, 640, True), (1536, 10240, 1280, True), (1536, 1280, 1280, False),
                                         (6144, 640, 640, False)])
def test_linear_layernorm_folded(dt, M, N, K, geglu, variant, monkeypatch):
    """consumer side: y = LN(x) W^T + b computed as rstd (x W'^T - mean colsum) + b' from the row sums the PRODUCER of x left
    (here: an identity-free producer GEMM x = x0 W0^T + residual so that the slab layout is the real one); reference = torch layer_norm +
    matmul in fp64 on the same rounded x and the UNfolded weights.  variant 0: the LEAN fold of round 5 (k_gemm8<.., LNV = 1 | 2>, the
    persistent k_gemm8p<.., 2> for the multi-round GEGLU shapes, the 64-row two-workgroups-per-CU tile for the K = N = C shapes); GC_GEMM_VAR_NO_LEAN_LN: the
    round-2 everything-epilogue (FUSE), kept as the fallback of split-K / statistics-carrying problems."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import _fold_ln, geglu_permute
    monkeypatch.setattr(ops, "OPTIONS", dataclasses.replace(ops.OPTIONS, gemm_variant=ops.OPTIONS.gemm_variant | variant))
    x0 = _rand((M, 256), dt, 1.0, 1); w0 = _rand((K, 256), dt, 256 ** -0.5 * 1.7, 5); b0 = torch.full((K,), 0.4, device=DEV)
    res = _rand((M, K), dt, 0.7, 9)
    rs = ops.RowStats()
    x = ops.linear(x0, w0, b0, residual=res, row_stats=rs)                     # producer (bias + residual): leaves the row sums of x
    assert torch.equal(x, ops.linear(x0, w0, b0, residual=res))                # ... and the same values as without the statistics
    # the partial sums themselves: summed over the slots = (sum, sum^2) of the row as stored
    tot = rs.buf.double().sum(0)
    assert float((tot[:, 0] - x.double().sum(1)).abs().max()) <= 1e-4 * float(x.double().abs().sum(1).max())
    assert float((tot[:, 1] - (x.double() ** 2).sum(1)).abs().max()) <= 1e-4 * float((x.double() ** 2).sum(1).max())
    w32 = torch.randn(N, K, generator=torch.Generator().manual_seed(2)).to(DEV) * K ** -0.5
    b = torch.randn(N, device=DEV); gamma = 1 + 0.2 * torch.randn(K, device=DEV); beta = 0.3 * torch.randn(K, device=DEV)
    o = {}
    _fold_ln(o, "w", w32, b, gamma, beta, dt)
    wf, bf = o["w.weight"], o["w.bias"]
    # the fold itself is exact algebra (tests/test_oracle_sd.py::test_layernorm_fold_algebra): LN(x) W^T + b == z (W diag(gamma))^T + b + W beta
    # with z = (x - mean) rstd.  The kernel is checked against that expression with the ROUNDED folded weights it actually multiplies.
    z = F.layer_norm(x.double(), (K,), None, None, 1e-5)
    ref = z @ wf.double().T + bf.double()
    full = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5) @ w32.double().T + b.double()
    assert float((ref - full).norm() / full.norm()) < 3 * EPS[dt]          # fold + one weight rounding stays at rounding level overall
    if geglu:
        hid, gate = ref.chunk(2, dim=-1)
        ref = hid * F.gelu(gate)
        wf, bf = geglu_permute(wf, bf)
    colsum = wf.float().sum(1).contiguous()
    got = ops.linear(x, wf, bf, geglu=geglu, ln=(rs, colsum, 1e-5))
    _close(got, ref, dt, extra=2.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("variant", [0, GC_GEMM_VAR_NO_LEAN_LN])
@pytest.mark.parametrize("B,L,C", [(6, 1024, 640), (6, 256, 1280), (2, 64, 1280)])
def test_qkv_transposed_v_with_layernorm_folded(dt, B, L, C, variant, monkeypatch):
    """the fused Q | K | V^T projection (columns [0, 2C) -> qk, [2C, 3C) -> V^T [B, C, Lp]) as a LayerNorm-FOLDED consumer: norm1 of a C = 640 /
    1280 transformer block (diffusers BasicTransformerBlock.norm1 -> attn1.to_q/k/v) inside the GEMM's plain epilogue, the row statistics from
    the proj_in-like producer's lean epilogue"""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import _fold_ln
    monkeypatch.setattr(ops, "OPTIONS", dataclasses.replace(ops.OPTIONS, gemm_variant=ops.OPTIONS.gemm_variant | variant))
    x0 = _rand((B, L, C), dt, 1.0, 1); w0 = _rand((C, C), dt, C ** -0.5 * 1.5, 5); b0 = torch.full((C,), -0.2, device=DEV)
    rs = ops.RowStats()
    x = ops.linear(x0, w0, b0, row_stats=rs)
    w32 = torch.randn(3 * C, C, generator=torch.Generator().manual_seed(2)).to(DEV) * C ** -0.5
    gamma = 1 + 0.2 * torch.randn(C, device=DEV); beta = 0.3 * torch.randn(C, device=DEV)
    o = {}
    _fold_ln(o, "w", w32, None, gamma, beta, dt)
    wf, bf = o["w.weight"], o["w.bias"]
    colsum = wf.float().sum(1).contiguous()
    ref = F.layer_norm(x.double(), (C,), None, None, 1e-5) @ wf.double().T + bf.double()
    Lp = (L + 7) // 8 * 8
    vt = torch.zeros(B, C, Lp, dtype=dt, device=DEV)
    qk = ops.linear(x, wf, bf, rows_per_batch=L, out_t=vt, ldt=Lp, t_batch_stride=C * Lp, t_col0=2 * C, out_cols=2 * C, ln=(rs, colsum, 1e-5))
    _close(qk, ref[..., :2 * C], dt, extra=2.0)
    _close(vt[..., :L].transpose(1, 2), ref[..., 2 * C:], dt, extra=2.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,L,C", [(6, 1024, 640), (6, 256, 1280), (6, 64, 1280), (8, 256, 1280), (2, 1024, 640)])
def test_text_cross_attention_folded_into_two_gemms(dt, B, L, C):
    """attn2 of a LayerNorm-folded transformer block -- norm2 -> to_q -> softmax(q K_text^T / sqrt(D)) V_text -> to_out + bias + residual (diffusers
    BasicTransformerBlock.attn2 behind /root/reference/gaussctrl/gc_pipeline.py:209-219; one text row per CFG half) -- as TWO GEMMs with one weight
    set per half (SDNet._text_fold): scores = LN(x) (K Wq)^T with the per-head softmax in the epilogue (k_gemm8<.., LNV = 3>), then P (Wo V^T)^T +
    b + x.  Reference: the unfolded chain in float64 on the same rounded x, text K / V^T and weights.  The fold replaces the bf16 rounding of q and
    of the attention output by ONE rounding of the folded matrices and of P: bar = 4 output roundings (as the attention kernels' tests)."""
    import math
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.unet import AttnCtx, SDNet
    from gaussctrl_amd.sd.weights import LOG2E, _fold_ln
    heads, Lt, Dc = 8, 77, 768
    D = C // heads
    t = "blk"
    g = torch.Generator().manual_seed(4)
    r = lambda *shp, sc=1.0: (torch.randn(*shp, generator=g) * sc).to(DEV)
    wq32, wk, wv, wo = r(C, C, sc=C ** -0.5), r(C, Dc, sc=Dc ** -0.5).to(dt), r(C, Dc, sc=Dc ** -0.5).to(dt), r(C, C, sc=C ** -0.5).to(dt)
    bo = r(C, sc=0.2); gamma = 1 + 0.2 * r(C); beta = 0.3 * r(C)
    w = {}
    _fold_ln(w, t + ".attn2.to_q", wq32 * (D ** -0.5 * LOG2E), None, gamma, beta, dt)          # W' = Wq diag(gamma) (prescaled), b' = Wq beta, colsum
    w.update({t + ".attn2.to_k.weight": wk, t + ".attn2.to_v.weight": wv, t + ".attn2.to_out.0.weight": wo, t + ".attn2.to_out.0.bias": bo})
    net = object.__new__(SDNet)
    net.w, net.cfg = w, {"heads": heads}
    ctx = r(2, Lt, Dc).to(dt)
    actx = AttnCtx("xview", 0.6, B // 2, {}, None, "unet")
    tf = net._text_fold(t, ctx, actx)
    assert tf is not None
    A, a, acs, Bm, bo2, lt = tf
    assert A.shape == (2, 640, C) and Bm.shape == (2, C, 640) and lt == Lt
    # producer of x: a GEMM + residual that leaves the row partials, as attn1.to_out does
    x0 = _rand((B, L, 256), dt, 1.0, 1); w0 = _rand((C, 256), dt, 256 ** -0.5 * 1.5, 5); res = _rand((B, L, C), dt, 0.8, 9)
    rs = ops.RowStats()
    x = ops.linear(x0, w0, torch.full((C,), 0.3, device=DEV), residual=res, row_stats=rs)
    Mh = (B // 2) * L
    pr = ops.linear(x, A, a, ln=(rs, acs, 1e-5), w_set_rows=Mh, softmax_keys=Lt)
    rs3 = ops.RowStats()
    out = ops.linear(pr, Bm, bo2, residual=x, row_stats=rs3, w_set_rows=Mh)
    # float64 reference of the unfolded chain
    k, vt, _ = net._text_kv(t + ".attn2", ctx, actx)                       # the rounded text K [2, Lt, C] / V^T [2, C, Lp] the product uses
    z = F.layer_norm(x.double(), (C,), None, None, 1e-5)
    q = z @ w[t + ".attn2.to_q.weight"].double().T + w[t + ".attn2.to_q.bias"].double()            # carries log2(e) / sqrt(D)
    q = q.view(2, B // 2, L, heads, D)
    kk = k.double().view(2, Lt, heads, D); vv = vt.double()[:, :, :Lt].transpose(1, 2).reshape(2, Lt, heads, D)
    sc = torch.einsum("gblhd,gjhd->gblhj", q, kk) * math.log(2.0)          # natural-log scores
    p = torch.softmax(sc, -1)
    o = torch.einsum("gblhj,gjhd->gblhd", p, vv).reshape(B, L, C)
    ref = o @ wo.double().T + bo.double() + x.double()
    # the probabilities themselves: rows sum to one over the 77 keys, zero in the padding columns
    prd = pr.double().view(B, L, heads, 80)
    assert float(prd[..., Lt:].abs().max()) == 0.0
    within("softmax rows sum to 1", float((prd[..., :Lt].sum(-1) - 1).abs().max()), 4 * EPS[dt])
    within("probabilities vs float64", float((prd[..., :Lt] - p.reshape(B, L, heads, Lt)).abs().max()), 3 * EPS[dt])
    _close(out, ref, dt, extra=4.0)
    tot = rs3.buf.double().sum(0)
    assert float((tot[:, 0] - out.double().reshape(-1, C).sum(1)).abs().max()) <= 1e-4 * float(out.double().abs().reshape(-1, C).sum(1).max())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,HW,C,G", [(2, 256, 320, 32), (3, 64, 1280, 32), (2, 112, 2560, 32), (6, 4096, 320, 32), (2, 36, 960, 32), (1, 16, 1920, 32)])
def test_groupnorm_apply_from_statistics(dt, B, HW, C, G):
    from gaussctrl_amd.sd import ops
    x = (_rand((B, HW, C), dt, 1.0, 1).float() * 2 + 1.0).to(dt)
    gamma = torch.randn(C, device=DEV); beta = torch.randn(C, device=DEV)
    gs = _group_sums(x, G).float().contiguous()
    ref = F.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), 1e-6).transpose(1, 2)
    _close(ops.groupnorm_apply(x, gs, gamma, beta, G, 1e-6, False), ref, dt, extra=2.0)
    _close(ops.groupnorm_apply(x, gs, gamma, beta, G, 1e-6, True), F.silu(ref), dt, extra=2.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,HW,C1,C2", [(2, 256, 640, 320), (3, 64, 1280, 1280), (6, 1024, 320, 320), (2, 100, 1280, 640)])
def test_concat_add_with_statistics(dt, B, HW, C1, C2):
    from gaussctrl_amd.sd import ops
    a = _rand((B, HW, C1), dt, 1.0, 1); b = _rand((B, HW, C2), dt, 1.0, 2); c = _rand((B, HW, C2), dt, 1.0, 3)
    for cc in (c, None):
        gs = torch.zeros(B, 32, 2, device=DEV)
        out = ops.concat_add(a, b, cc, group_stats=gs)
        assert torch.equal(out, ops.concat_add(a, b, cc))
        _stats_close(gs, _group_sums(out, 32), _group_sums_abs(out, 32))


# ------------------------------------------------------------------------------------------- fp8 (e4m3, block-scaled MFMA)
def _deq(q8, scale_bytes=None):
    v = q8.view(torch.float8_e4m3fn).double()
    return v if scale_bytes is None else v * torch.exp2(scale_bytes.double() - 127)[:, None]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(2, 16, 16, 128, 128, 1), (6, 64, 64, 320, 320, 1), (2, 32, 32, 640, 640, 1), (3, 16, 16, 1280, 640, 1),
                                                   (2, 32, 32, 320, 320, 2), (2, 8, 8, 960, 320, 1), (1, 24, 20, 256, 96, 1)])
def test_conv3x3_fp8(dt, B, H, W, Cin, Cout, stride):
    """k_gemm8q vs the fp64 convolution of the SAME e4m3 operands (dequantised on the host): the kernel's only error sources are the
    fp32 accumulation order and the output rounding."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight_fp8
    g = torch.Generator().manual_seed(1)
    Cp = ops.pad128(Cin)
    x32 = torch.randn(B, H, W, Cin, generator=g) * 1.5
    x8 = torch.zeros(B, H, W, Cp, dtype=torch.uint8)
    x8[..., :Cin] = x32.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    w32 = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    w8, wsc = conv3x3_weight_fp8(w32)
    b = torch.randn(w8.shape[0], generator=g)
    for a_scale in (127, 125):
        xr = _deq(x8)[..., :Cin] * 2.0 ** (a_scale - 127)
        wr = _deq(w8, wsc).reshape(-1, 3, 3, Cp)[:Cout, :, :, :Cin].permute(0, 3, 1, 2)
        ref = F.conv2d(xr.permute(0, 3, 1, 2), wr, b[:Cout].double(), stride=stride, padding=1).permute(0, 2, 3, 1)
        gs = torch.zeros(B, 32, 2, device=DEV) if w8.shape[0] % 32 == 0 and (ref.shape[1] * ref.shape[2]) % 16 == 0 else None
        got = ops.conv3x3_fp8(on_device(x8, DEV), on_device(w8, DEV), on_device(wsc, DEV), dt, on_device(b, DEV), stride=stride, a_scale=a_scale, group_stats=gs)
        _close(got[..., :Cout], ref, dt)
        if gs is not None and w8.shape[0] == Cout:
            _stats_close(gs, _group_sums(got.reshape(B, -1, Cout), 32), _group_sums_abs(got.reshape(B, -1, Cout), 32))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(256, 320, 384), (24576, 320, 1280), (1000, 1280, 640), (384, 1280, 5120)])
def test_linear_fp8(dt, M, N, K):
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import quantize_rows_e4m3
    g = torch.Generator().manual_seed(2)
    x8 = (torch.randn(M, K, generator=g) * 2).to(torch.float8_e4m3fn).view(torch.uint8)
    w8, wsc = quantize_rows_e4m3(torch.randn(N, K, generator=g) * K ** -0.5)
    b = torch.randn(N, generator=g); r = _rand((M, N), dt, 1.0, 3)
    ref = _deq(x8) @ _deq(w8, wsc).T + b.double()
    got = ops.linear_fp8(on_device(x8, DEV), on_device(w8, DEV), on_device(wsc, DEV), dt, on_device(b, DEV), residual=r)
    _close(got, ref + r.double().cpu(), dt)


def _e4m3_bytes_match(y8, want_real, a_scale, max_frac):
    """y8 (uint8, e4m3 of value * 2^(127 - a_scale)) equals the e4m3 rounding of `want_real` (fp64): a share < max_frac of the bytes may sit
    ONE e4m3 step away (the kernel's fp32 arithmetic lands on the other side of a rounding boundary), none further."""
    q = 2.0 ** (a_scale - 127)
    got = y8.view(torch.float8_e4m3fn).double().cpu() * q
    want = (want_real.cpu() / q).clamp(-448, 448).float().to(torch.float8_e4m3fn).double() * q
    diff = (got - want).abs()
    within("share of e4m3 bytes that differ from the rounded fp64 result", float((diff > 0).double().mean()), max_frac)
    assert bool((diff <= torch.maximum(0.126 * want.abs(), torch.tensor(2.0 ** -9 * q).double()) + 1e-12).all()), float(diff.max())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,C", [(1024, 640), (384, 1280), (1001, 1280), (64, 320)])
def test_layernorm_fp8(dt, M, C):
    """LayerNorm with an e4m3 output (gc_dn_layernorm_fp8): the e4m3 rounding of the fp64 LayerNorm of the same input."""
    from gaussctrl_amd.sd import ops
    x = (_rand((M, C), dt, 1.0, 1).float() * 1.7 + 0.4).to(dt)
    gamma = torch.randn(C, device=DEV) * 0.5 + 1.0; beta = torch.randn(C, device=DEV) * 0.3
    ref = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), 1e-5)
    for a_scale in (127, 125):
        y8 = ops.layernorm_fp8(x, gamma, beta, 1e-5, a_scale)
        assert y8.shape == x.shape and y8.dtype == torch.uint8
        _e4m3_bytes_match(y8, ref, a_scale, 2e-3)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K", [(1024, 5120, 640), (384, 10240, 1280), (1000, 2560, 640), (6144, 5120, 640)])
def test_linear_fp8_geglu_and_e4m3_output(dt, M, N, K):
    """the GEGLU projection on e4m3 operands (k_gemm8q, rows permuted by weights.geglu_permute): 2-byte output vs fp64 of the same operands,
    and the e4m3 output (gc_gemm_desc.out_fp8) vs the e4m3 rounding of that fp64 result; then the FF down projection consumes the bytes."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import quantize_rows_e4m3, geglu_permute
    g = torch.Generator().manual_seed(4)
    x8 = (torch.randn(M, K, generator=g) * 1.5).to(torch.float8_e4m3fn).view(torch.uint8)
    w32 = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.5
    w8, wsc = quantize_rows_e4m3(w32)
    full = _deq(x8) @ _deq(w8, wsc).T + b.double()
    ref = full[:, :N // 2] * F.gelu(full[:, N // 2:])
    wp, bp = geglu_permute(w8, b)
    scp, _ = geglu_permute(wsc, None)
    got = ops.linear_fp8(x8.to(DEV), wp.to(DEV), scp.to(DEV), dt, bp.to(DEV), geglu=True)
    assert got.shape == (M, N // 2)
    # GEGLU multiplies two accumulators: the accumulation noise `_close` grants ONE accumulator (5 % of a rounding of the largest value; the
    # block-scaled MFMA uses 0.64 of it on a plain fp8 linear in f16, test_linear_fp8) reaches the output times |gelu(gate)| + |x| |gelu'(gate)|
    hid, gate = full[:, :N // 2], full[:, N // 2:]
    tol = EPS[dt] * 2.0
    acc = tol * float(full.abs().max()) * 0.05
    slack = acc * (float(F.gelu(gate).abs().max()) + 1.13 * float(hid.abs().max())) + 1e-6
    err = (got.double().cpu() - ref).abs()
    within("GEGLU output: (err - one rounding) / propagated accumulation slack", ((err - tol * ref.abs()) / slack).clamp_min(0).max().item(), 1.0)
    for osc in (127, 126):
        y8 = ops.linear_fp8(x8.to(DEV), wp.to(DEV), scp.to(DEV), dt, bp.to(DEV), geglu=True, out_fp8=osc)
        assert y8.dtype == torch.uint8 and y8.shape == (M, N // 2)
        _e4m3_bytes_match(y8, ref, osc, 5e-3)
        # the down projection on those bytes (a_scale = the producer's out_fp8)
        w2, w2sc = quantize_rows_e4m3(torch.randn(K, N // 2, generator=g) * (N // 2) ** -0.5)
        r = _rand((M, K), dt, 1.0, 5)
        a2, wd2 = _deq(y8.cpu()) * 2.0 ** (osc - 127), _deq(w2, w2sc)
        ref2 = a2 @ wd2.T + r.double().cpu()
        got2 = ops.linear_fp8(y8, w2.to(DEV), w2sc.to(DEV), dt, residual=r, a_scale=osc).double().cpu()
        # the GEGLU hidden is heavy-tailed (a few values of 30 .. 50 among many below 1) and K = 4C is long: what the block-scaled MFMA loses while
        # it aligns 128 products per instruction scales with sum_k |a_k w_k|, not with the output -- bound it there: one output rounding +
        # 2^-14 of the magnitude sum (measured 2^-17.3 .. 2^-15.6 on MI355X; an ideal fp32 accumulation would sit near sqrt(K) 2^-24 ~ 2^-18)
        mag = a2.abs() @ wd2.abs().T + r.double().cpu().abs()
        within("fp8 down projection: (err - one rounding) / (2^-14 sum |a w|)",
               (((got2 - ref2).abs() - EPS[dt] * ref2.abs()).clamp_min(0) / (2.0 ** -14 * mag)).max().item(), 1.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,L,C", [(2, 1024, 640), (3, 256, 1280), (2, 64, 1280), (1, 100, 640)])
def test_linear_fp8_qkv_transposed_v(dt, B, L, C):
    """the fused Q | K | V projection on e4m3 operands: columns [0, 2C) -> qk [B, L, 2C], columns [2C, 3C) -> V^T [B, C, Lp] (the layout of
    ops.linear(out_t=...) the attention kernels read)."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import quantize_rows_e4m3
    g = torch.Generator().manual_seed(6)
    x8 = (torch.randn(B, L, C, generator=g) * 1.5).to(torch.float8_e4m3fn).view(torch.uint8)
    w8, wsc = quantize_rows_e4m3(torch.randn(3 * C, C, generator=g) * C ** -0.5)
    ref = _deq(x8) @ _deq(w8, wsc).T
    Lp = (L + 7) // 8 * 8
    vt = torch.zeros(B, C, Lp, dtype=dt, device=DEV)
    qk = ops.linear_fp8(on_device(x8, DEV), on_device(w8, DEV), on_device(wsc, DEV), dt, rows_per_batch=L, out_t=vt, ldt=Lp, t_batch_stride=C * Lp, t_col0=2 * C,
                        out_cols=2 * C)
    assert qk.shape == (B, L, 2 * C)
    _close(qk, ref[..., :2 * C], dt)
    _close(vt[..., :L].transpose(1, 2), ref[..., 2 * C:], dt)
    if Lp != L:
        assert float(vt[..., L:].abs().max()) == 0.0


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind,B,H,Cin,Cout", [("linear", 6, 64, 320, 320), ("linear", 2, 32, 640, 640), ("conv", 6, 16, 1280, 1280), ("concat", 6, 64, 320, 640),
                                               ("concat", 2, 32, 640, 640), ("concat", 2, 18, 320, 320)])
def test_groupnorm_apply_parts_fp8(dt, kind, B, H, Cin, Cout):
    """GroupNorm + SiLU -> e4m3 in ONE launch from the partial sums the producer of the tensor left (gc_dn_groupnorm_apply_parts_fp8): the
    e4m3 rounding of the fp64 GroupNorm of the stored tensor; channel counts that pad to 128 (320 -> 384, 960 -> 1024) have zero padding."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight
    if kind == "linear":
        x = _rand((B, H * H, Cin), dt, 1.0, 1); w = _rand((Cout, Cin), dt, Cin ** -0.5, 2); b = torch.randn(Cout, device=DEV) + 0.7
        out, parts = ops.linear(x, w, b, rows_per_batch=H * H, chan_parts=True)
    elif kind == "conv":
        x = _rand((B, H, H, Cin), dt, 1.0, 1); w = _rand((Cout, Cin, 3, 3), dt, (9 * Cin) ** -0.5, 2); b = torch.randn(Cout, device=DEV) + 0.7
        out, parts = ops.conv3x3(x, conv3x3_weight(w, dt), b, chan_parts=True)
    else:
        a = (_rand((B, H, H, Cin), dt, 1.0, 1).float() + 1.0).to(dt); bb = _rand((B, H, H, Cout), dt, 1.0, 2)
        out, parts = ops.concat_add(a, bb, None, chan_parts=True)
    if parts is None and ops.OPTIONS.gemm_variant:
        pytest.skip("a forced kernel variant without the statistics epilogue")
    assert parts is not None
    Co = out.shape[-1]
    o64 = out.double().reshape(B, -1, Co)
    gamma = torch.randn(Co, device=DEV) * 0.5 + 1.0; beta = torch.randn(Co, device=DEV) * 0.5
    ref = F.silu(F.group_norm(o64.transpose(1, 2), 32, gamma.double(), beta.double(), 1e-5).transpose(1, 2))
    for a_scale in (127, 126):
        y8 = ops.groupnorm_apply_parts_fp8(out, parts, gamma, beta, 32, 1e-5, True, a_scale)
        Cp = ops.pad128(Co)
        assert y8.shape == out.shape[:-1] + (Cp,) and (Cp == Co or int(y8[..., Co:].max()) == 0)
        _e4m3_bytes_match(y8.reshape(B, -1, Cp)[..., :Co], ref, a_scale, 2e-3)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,H,Cin,Cout", [(6, 16, 1280, 1280), (6, 16, 2560, 1280), (3, 16, 640, 1280), (14, 16, 1280, 1280), (6, 16, 1920, 1280),
                                          (6, 64, 320, 320), (6, 32, 640, 640), (2, 32, 1280, 640), (3, 64, 640, 320), (6, 32, 960, 640)])
def test_conv3x3_fp8_k_sliced_with_partials(dt, B, H, Cin, Cout):
    """the resnet convolutions on e4m3 operands WITH the GroupNorm partials of their output: 16 x 16 maps at small batch run k_gemm8q in
    k-slices + the split-K reduce kernel of the 2-byte path (which leaves the partials); everything else runs k_gemm8q's own channel-partial
    epilogue (tiles of 128 / 192 rows that straddle batches, column tiles of 128 / 160) -- output vs fp64 of the same operands, identical to
    the plain launch, partials vs the stored output, and the one-launch e4m3 GroupNorm that follows."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight_fp8
    g = torch.Generator().manual_seed(7)
    Cp = ops.pad128(Cin)
    x8 = torch.zeros(B, H, H, Cp, dtype=torch.uint8)
    x8[..., :Cin] = (torch.randn(B, H, H, Cin, generator=g) * 1.5).to(torch.float8_e4m3fn).view(torch.uint8)
    w32 = torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5
    w8, wsc = conv3x3_weight_fp8(w32)
    b = torch.randn(Cout, generator=g) + 0.5
    rv = torch.randn(1, Cout, generator=g).to(DEV)
    res = _rand((B, H, H, Cout), dt, 1.0, 3)
    wr = _deq(w8, wsc).reshape(-1, 3, 3, Cp)[:Cout, :, :, :Cin].permute(0, 3, 1, 2)
    ref = F.conv2d(_deq(x8)[..., :Cin].permute(0, 3, 1, 2), wr, b.double(), padding=1).permute(0, 2, 3, 1) + rv.double().cpu() + res.double().cpu()
    out, parts = ops.conv3x3_fp8(x8.to(DEV), w8.to(DEV), wsc.to(DEV), dt, b.to(DEV), rowvec=rv, ld_rowvec=0, residual=res, chan_parts=True)
    _close(out, ref, dt)
    plain = ops.conv3x3_fp8(x8.to(DEV), w8.to(DEV), wsc.to(DEV), dt, b.to(DEV), rowvec=rv, ld_rowvec=0, residual=res)
    assert torch.equal(out, plain)
    assert parts is not None, "every resnet convolution of the fp8 path leaves the partials of its output"
    if B * H * H <= 128 * 12 and H == 16 and not ops.OPTIONS.gemm_variant:      # (a forced tile height, tests/test_gemm_variants_gpu.py, does not slice)
        assert parts.rows == 32 and parts.col_tile == 64, "a part-filled grid with a long K must take the k-sliced path"
    if parts is not None:
        G, cpg = 32, Cout // 32
        o64 = out.double().reshape(B, H * H, Cout)
        for bi in range(B):
            got = _parts_sums(parts, bi, H * H, cpg)
            og = o64[bi].reshape(H * H, G, cpg)
            want = torch.stack([og.sum((0, 2)), (og ** 2).sum((0, 2))], -1)
            within("fp8 conv: group partial sums vs fp64 (rel to sum |x| resp. sum x^2)",
                   ((got - want).abs() / torch.stack([og.abs().sum((0, 2)), (og ** 2).sum((0, 2))], -1).clamp_min(1e-6)).max().item(), 2e-6)
        gamma = torch.randn(Cout, device=DEV) * 0.5 + 1.0; beta = torch.randn(Cout, device=DEV) * 0.5
        refn = F.silu(F.group_norm(o64.transpose(1, 2), 32, gamma.double(), beta.double(), 1e-5).transpose(1, 2))
        y8 = ops.groupnorm_apply_parts_fp8(out, parts, gamma, beta, 32, 1e-5, True, 127)
        _e4m3_bytes_match(y8.reshape(B, H * H, -1)[..., :Cout], refn, 127, 2e-3)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,HW,C", [(2, 256, 320), (3, 64, 1280), (6, 4096, 320), (2, 1024, 960)])
def test_groupnorm_apply_fp8(dt, B, HW, C):
    """GroupNorm + SiLU with e4m3 output: equals the e4m3 rounding of the fp32 result (ties / 1-ulp-of-fp8 differences allowed on < 1e-3
    of the values: the fp32 normalisation differs from the fp64 reference in the last bit); padding channels are zero."""
    from gaussctrl_amd.sd import ops
    x = (_rand((B, HW, C), dt, 1.0, 1).float() * 2 + 0.5).to(dt)
    gamma = torch.randn(C, device=DEV); beta = torch.randn(C, device=DEV)
    gs = _group_sums(x, 32).float().contiguous()
    ref = F.silu(F.group_norm(x.double().transpose(1, 2), 32, gamma.double(), beta.double(), 1e-5).transpose(1, 2))
    for a_scale in (127, 126):
        y8 = ops.groupnorm_apply_fp8(x, gs, gamma, beta, 32, 1e-5, True, a_scale)
        Cp = ops.pad128(C)
        assert y8.shape == (B, HW, Cp) and (Cp == C or int(y8[..., C:].max()) == 0)
        got = y8[..., :C].view(torch.float8_e4m3fn).double().cpu() * 2.0 ** (a_scale - 127)
        want = (ref.cpu() * 2.0 ** (127 - a_scale)).clamp(-448, 448).float().to(torch.float8_e4m3fn).double() * 2.0 ** (a_scale - 127)
        diff = (got - want).abs()
        assert float((diff > 0).double().mean()) < 2e-3
        # at most ONE e4m3 step: 2^-3 relative in the normal range, 2^-9 (x the tensor scale) in the subnormal range
        assert bool((diff <= torch.maximum(0.126 * want.abs(), torch.tensor(2.0 ** -9 * 2.0 ** (a_scale - 127)).double()) + 1e-12).all())


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,HW,C", [(6, 4096, 320), (2, 1024, 1920), (3, 256, 2560), (2, 100, 960)])
def test_group_stats_then_apply(dt, B, HW, C):
    """the two-launch stand-alone GroupNorm: gc_dn_group_stats (atomics into zeroed [B,G,2]) + gc_dn_groupnorm_apply"""
    from gaussctrl_amd.sd import ops
    x = (_rand((B, HW, C), dt, 1.0, 1).float() * 1.5 + 0.8).to(dt)
    gamma = torch.randn(C, device=DEV); beta = torch.randn(C, device=DEV)
    gs = ops.group_stats(x, torch.zeros(B, 32, 2, device=DEV))
    _stats_close(gs, _group_sums(x, 32), _group_sums_abs(x, 32))
    ref = F.silu(F.group_norm(x.double().transpose(1, 2), 32, gamma.double(), beta.double(), 1e-5).transpose(1, 2))
    _close(ops.groupnorm_apply(x, gs, gamma, beta, 32, 1e-5, True), ref, dt, extra=2.0)


@pytest.mark.parametrize("dt", DTS)
def test_tile_order_does_not_change_results(dt, monkeypatch):
    """The GEMM's workgroup -> (tile, k-slice) assignment (column panels per XCD, XCD-owned k-slices: dn_gemm_kernels.h tile_coords / wg_tile) is a
    pure scheduling choice: forced panel widths 0 (whole rows) / 1 / 3 / 7 give bit-identical outputs to the automatic choice on a short-K linear,
    the persistent GEGLU projection, a k-sliced linear, 16 x 16 / 8 x 8-map convolutions (k-slices on both kernel families)."""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import geglu_permute, conv3x3_weight

    def cases():
        x = _rand((1536, 1280), dt, 1.0, 1); w = _rand((1280, 1280), dt, 1280 ** -0.5, 2); b = _rand((1280,), torch.float32, 1.0, 20)
        yield "linear", lambda: ops.linear(x, w, b, residual=x)
        wg, bg = geglu_permute(_rand((10240, 1280), dt, 1280 ** -0.5, 3), _rand((10240,), torch.float32, 1.0, 21))
        yield "geglu persistent", lambda: ops.linear(x, wg, bg, geglu=True)
        x5 = _rand((1536, 6400), dt, 1.0, 4); w5 = _rand((1280, 6400), dt, 6400 ** -0.5, 5)
        yield "k-sliced linear", lambda: ops.linear(x5, w5, b)
        xq = _rand((6, 1024, 640), dt, 1.0, 6); wq = _rand((1920, 640), dt, 640 ** -0.5, 7)
        yield "wide linear", lambda: ops.linear(xq, wq)
        for H in (16, 8):
            xc = _rand((6, H, H, 1280), dt, 1.0, 8 + H); wc = conv3x3_weight(_rand((1280, 1280, 3, 3), dt, (9 * 1280) ** -0.5, 9), dt)
            bc = _rand((1280,), torch.float32, 1.0, 22)
            yield f"conv {H}x{H}", lambda xc=xc, wc=wc, bc=bc: ops.conv3x3(xc, wc, bc)

    base = {}
    for name, fn in cases():
        o = fn(); base[name] = (o[0] if isinstance(o, tuple) else o).clone()
    for pw in (0, 1, 3, 7):
        monkeypatch.setattr(ops, "OPTIONS", dataclasses.replace(ops.OPTIONS, gemm_variant=(pw + 1) << ops.GC_GEMM_VAR_PW_SHIFT))
        for name, fn in cases():
            o = fn(); o = o[0] if isinstance(o, tuple) else o
            assert torch.equal(o, base[name]), (name, pw)


@pytest.mark.parametrize("dt", DTS)
def test_attention_head160_wide_form_matches_64_query_form(dt, monkeypatch):
    """k_attn_wide (head size 160, set-split: all 256 queries of a (frame, head) in one 8-wave workgroup, 32 queries per wave) runs the same body as
    the 64-query form (GC_ATTN_VAR_D160_Q64): per set the same keys in the same tile order -> bit-identical partial outputs and result."""
    from gaussctrl_amd.sd import ops
    f, L, heads, D = 5, 256, 8, 160
    B, C = 2 * f, heads * D
    q = _rand((B, L, C), dt, 1.0, 1); k = _rand((B, L, C), dt, 1.0, 2); v = _rand((B, L, C), dt, 1.0, 3)
    k[:, 37, :] = k[:, 37, :] * 5.0                       # a spiked key: the running maximum jumps inside the first tile
    vt = v.transpose(1, 2).contiguous()
    sets = [(-1, 0.6)] + [(r, 0.1) for r in range(4)]
    wide = ops.attention(q, k, vt, heads, sets, f, Lk=L)
    monkeypatch.setattr(ops, "OPTIONS", dataclasses.replace(ops.OPTIONS, attn_variant=ops.GC_ATTN_VAR_D160_Q64))
    narrow = ops.attention(q, k, vt, heads, sets, f, Lk=L)
    assert torch.equal(wide, narrow)


@pytest.mark.gpu
def test_gemm_refuses_operands_beyond_32bit_element_offsets():
    """the GEMM / conv kernels index an operand with 32-bit element offsets: a problem that does not fit is refused with an error code
    (round 6: a 42-view VAE decode batch, 2.8 G elements at 512 x 512 x 256, used to fault), and DenoisePipeline.decode groups its frames"""
    import ctypes as C
    from gaussctrl_amd import _lib as L
    from gaussctrl_amd.sd import ops
    x = torch.zeros(256, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(256, 64, dtype=torch.bfloat16, device=DEV)
    z = torch.zeros(64, dtype=torch.uint8, device=DEV)
    d = ops.GemmDesc()
    d.dtype = 0; d.mode = 0; d.M, d.N, d.K = 1 << 26, 64, 64          # M * lda = 2^32 elements (the tensors behind the pointers are small: nothing is launched)
    d.A = x.data_ptr(); d.lda = 64; d.W = w.data_ptr(); d.out = o.data_ptr(); d.ldc = 64; d.out_scale = 1.0; d.zeros = z.data_ptr()
    with pytest.raises(L.GaussCtrlHipError, match="32-bit"):
        L.check(L.lib().gc_dn_gemm(C.byref(d), C.c_void_p(ops.stream_handle())), "gc_dn_gemm")
    d.mode = 1; d.M = 48 * 512 * 512; d.B, d.Hi, d.Wi, d.Cin, d.Ho, d.Wo, d.stride, d.pad_lo = 48, 512, 512, 256, 512, 512, 1, 1; d.K = 9 * 256
    with pytest.raises(L.GaussCtrlHipError, match="32-bit"):
        L.check(L.lib().gc_dn_gemm(C.byref(d), C.c_void_p(ops.stream_handle())), "gc_dn_gemm")
    torch.cuda.synchronize()
