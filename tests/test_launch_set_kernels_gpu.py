"""GPU parity of the denoise kernels at the batches of a launch set (4 chunks share one UNet / ControlNet batch -- 24 CFG frames
at chunk_size 3, 12 for the short last set of a scene, 40 at the plugin's chunk_size 5), where the host code picks other kernels than at the
CFG batch <= 14 of tests/test_denoise_kernels_gpu.py: the 256-row k-sliced 8 x 8-map convs, 256-row unsliced 16 x 16-map convs, k_attn5 in 12
rounds, the set-split D = 160 forms.  Every case names the kernel it must have run (gc_dn_gemm_selection / gc_dn_attention_selection on the
descriptor as it went to the launch) and is compared with a float64 reference of the same op on the same rounded inputs, at the bars of
test_denoise_kernels_gpu.py.  The f16 edges of the static-offset attention kernels (offset overflow in one set of five, logit spreads, keys 14 - 16
binades below a sampled maximum) close the file."""
import math

import pytest
import torch
import torch.nn.functional as F

from test_abi import _LAUNCH_SET_CONVS
from test_denoise_kernels_gpu import DTS, _close, _rand
from test_denoise_kernels_gpu import test_groupnorm_from_producer_partials as _gn_from_parts
from test_denoise_kernels_gpu import test_linear_layernorm_folded as _ln_folded
from test_denoise_kernels_gpu import test_linear_persistent_multi_round as _persistent
from test_denoise_kernels_gpu import test_qkv_transposed_v_with_layernorm_folded as _qkv_folded
from test_denoise_kernels_gpu import test_text_cross_attention_folded_into_two_gemms as _text_folded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LN2 = math.log(2.0)


@pytest.fixture
def sel_log(monkeypatch):
    """(kind, M | batch, selection) of every GEMM / attention launch of the test"""
    from gaussctrl_amd.sd import ops
    log = []
    monkeypatch.setattr(ops, "SELECTION_LOG", log)
    return log


def _gemms(log, M=None):
    return [s for kind, m, s in log if kind == "gemm" and (M is None or m == M)]


def _attns(log):
    return [s for kind, _, s in log if kind == "attn"]


# ---------------------------------------------------------------------------------------------------------------- 3 x 3 convolutions

def _conv_ref(x, w, b, stride, chunk=8):
    """float64 3 x 3 conv (pad 1) of NHWC x as nine tap GEMMs, `chunk` images at a time -> [B, Ho, Wo, Cout]"""
    B, H, W, _ = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    wd = w.double()
    out = torch.empty(B, Ho, Wo, w.shape[0], dtype=torch.float64, device=x.device)
    for c0 in range(0, B, chunk):
        xp = F.pad(x[c0:c0 + chunk].double(), (0, 0, 1, 1, 1, 1))
        acc = b.double().expand(xp.shape[0], Ho, Wo, -1).clone()
        for dy in range(3):
            for dx in range(3):
                acc += xp[:, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride, :] @ wd[:, :, dy, dx].T
        out[c0:c0 + chunk] = acc
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", [24, 40])
@pytest.mark.parametrize("H,Cin,Cout,stride", [(64, 320, 320, 1), (32, 640, 640, 1), (16, 1280, 1280, 1), (16, 1280, 1280, 2), (8, 1280, 1280, 1),
                                               (8, 2560, 1280, 1)])
def test_conv3x3_at_launch_set_batches(dt, B, H, Cin, Cout, stride, sel_log):
    """bias + time-embedding row + residual, with the GroupNorm partials asked for as the UNet's resnets do; the kernel is the one
    tests/test_abi.py pins for this batch (B = 24, 8 x 8 maps and the 16 -> 8 downsample: 256-row tiles x 4 k-slices, four whole images per tile)"""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight
    Ho = (H - 1) // stride + 1
    x = _rand((B, H, H, Cin), dt, 1.0, 1)
    w = _rand((Cout, Cin, 3, 3), dt, (9 * Cin) ** -0.5, 2)
    b = torch.randn(Cout, device=DEV)
    rv = torch.randn(B, Cout, device=DEV); res = _rand((B, Ho, Ho, Cout), dt, 1.0, 3)
    out, parts = ops.conv3x3(x, conv3x3_weight(w, dt), b, stride=stride, rowvec=rv, residual=res, chan_parts=True)
    (s,) = _gemms(sel_log)
    want, lay, _ = _LAUNCH_SET_CONVS[(H, Cin, Cout, stride)][B]
    assert (s["kernel"], s["m_tiles"], s["splits"], s["ntw"]) == want, s
    assert (parts is None) == (lay is None) == (s["parts"] == 0), (s, lay)
    ref = _conv_ref(x, w, b, stride) + rv.double()[:, None, None, :] + res.double()
    _close(out, ref, dt)
    if parts is not None:
        assert (parts.rows, parts.nslab, parts.col_tile) == lay
        G, o64 = 32, out.double().reshape(B, Ho * Ho, Cout)
        gamma = torch.randn(Cout, device=DEV); beta = torch.randn(Cout, device=DEV)
        gref = F.group_norm(o64.transpose(1, 2), G, gamma.double(), beta.double(), 1e-5).transpose(1, 2).reshape(out.shape)
        _close(ops.groupnorm(out, gamma, beta, G, 1e-5, True, parts=parts), F.silu(gref), dt, extra=2.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B", [24, 40])
@pytest.mark.parametrize("kind,H,Cin,Cout", [("conv", 64, 320, 320), ("conv", 32, 640, 640), ("conv", 16, 1280, 1280), ("conv", 16, 2560, 1280),
                                             ("linear", 32, 640, 640), ("linear", 16, 1280, 1280), ("concat", 64, 320, 320)])
def test_groupnorm_from_partials_at_launch_set_batches(dt, B, kind, H, Cin, Cout, sel_log):
    """k_gn_apply_parts from the partials of the producer's epilogue at launch-set batches (256-row slabs: one slab per 16 x 16 map), through the
    checks of test_groupnorm_from_producer_partials (partial sums vs float64, GroupNorm(+SiLU) vs float64 and vs the stand-alone kernels)"""
    _gn_from_parts(dt, kind, B, H, Cin, Cout)
    if kind != "concat":
        s = _gemms(sel_log)[0]
        assert s["kernel"] == "k8" and s["m_tiles"] == 4 and s["parts"] == 2, s


# ---------------------------------------------------------------------------------------------------------------------------- linears

@pytest.mark.parametrize("dt", DTS)
def test_linear_persistent_at_launch_set_rows(dt, sel_log):
    """the level-0 GEGLU FF-up projection of a 24-frame set (M = 98 304): persistent workgroups, 30 tiles each"""
    _persistent(dt, 24 * 4096, 320, 2560, True)
    (s,) = _gemms(sel_log)
    assert s["kernel"] == "k8" and s["m_tiles"] == 4 and s["persist"] == 256, s


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("M,N,K,geglu,persist", [(24 * 1024, 640, 640, False, 256), (24 * 1024, 5120, 640, True, 256), (40 * 256, 10240, 1280, True, 256),
                                                 (24 * 64, 1280, 1280, False, 0)])
def test_linear_layernorm_folded_at_launch_set_rows(dt, M, N, K, geglu, persist, sel_log, monkeypatch):
    """the lean LayerNorm fold (consumer kind 2) at launch-set rows: persistent workgroups once the 256 x 128 tiles take more than one round,
    the 64-row two-workgroups-per-CU tile at the 8 x 8 level"""
    _ln_folded(dt, M, N, K, geglu, 0, monkeypatch)
    s = _gemms(sel_log)[-1]
    assert s["ln_kind"] == 2 and s["splits"] == 1 and s["persist"] == persist and s["m_tiles"] == (4 if persist else 1), s


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,L,C", [(24, 1024, 640), (24, 256, 1280), (40, 64, 1280)])
def test_qkv_transposed_v_at_launch_set_batches(dt, B, L, C, sel_log, monkeypatch):
    _qkv_folded(dt, B, L, C, 0, monkeypatch)
    s = _gemms(sel_log)[-1]
    assert s["ln_kind"] == 2 and s["kernel"] == "k8", s


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("B,L,C", [(24, 1024, 640), (40, 256, 1280), (24, 64, 1280)])
def test_text_cross_attention_fold_at_launch_set_batches(dt, B, L, C, sel_log):
    _text_folded(dt, B, L, C)
    g = _gemms(sel_log)
    assert any(s["ln_kind"] == 3 for s in g) and g[-1]["ln_kind"] == 1, g


# ------------------------------------------------------------------------------------------------------------------------ attention

SETS = [(-1, 0.6)] + [(r, 0.1) for r in range(4)]          # the product form: the view itself + its 4 references from the cached bank


def _attn_inputs(f, L, heads, D, seed, qscale=None, kscale=1.0):
    """prescaled Q' (scale * log2(e) folded in), K, V^T of 2 f frames and a reference bank of 2 x 4 frames"""
    B, C = 2 * f, heads * D
    q = _rand((B, L, C), torch.float32, 1.0, seed)
    qp = q * (D ** -0.5 * 1.4426950408889634 if qscale is None else qscale)
    k = _rand((B, L, C), torch.float32, kscale, seed + 1); v = _rand((B, L, C), torch.float32, 1.0, seed + 2)
    kr = _rand((8, L, C), torch.float32, kscale, seed + 3); vr = _rand((8, L, C), torch.float32, 1.0, seed + 4)
    return qp, k, v, kr, vr


def _sample_rows(B, L, seed, per=1, blk=64):
    """per frame: `per` random query rows in every block of `blk` queries -- every workgroup of every kernel (query blocks of 64 or 256), every
    round including the last -> LongTensor [B, S]"""
    g = torch.Generator().manual_seed(seed)
    nb = (L + blk - 1) // blk
    rows = torch.arange(nb).repeat_interleave(per)[None, :] * blk + torch.randint(0, blk, (B, nb * per), generator=g)
    return rows.clamp_max(L - 1).to(DEV)


def _ref_rows(qp, k, v, kr, vr, sets, f, heads, rows, chunk=8):
    """float64 sum_s w_s softmax(ln 2 * Q' K_s^T) V_s of the sampled rows [B, S] -> [B, S, C]"""
    B, L, C = qp.shape
    D = C // heads
    S = rows.shape[1]
    out = torch.zeros(B, S, C, dtype=torch.float64, device=qp.device)
    for c0 in range(0, B, chunk):
        bs = torch.arange(c0, min(B, c0 + chunk), device=qp.device)
        qs = torch.gather(qp[bs], 1, rows[bs][..., None].expand(-1, -1, C)).double().view(len(bs), S, heads, D)
        for kind, w in sets:
            if kind == -1:
                kk, vv = k[bs], v[bs]
            else:
                idx = (bs // f) * 4 + kind
                kk, vv = kr[idx], vr[idx]
            kk = kk.double().view(len(bs), -1, heads, D); vv = vv.double().view(len(bs), -1, heads, D)
            p = (torch.einsum("bshd,blhd->bhsl", qs, kk) * LN2).softmax(-1)
            out[bs] += w * torch.einsum("bhsl,blhd->bshd", p, vv).reshape(len(bs), S, C)
    return out


def _run_attn(dt, qp, k, v, kr, vr, f, heads, sets=SETS):
    from gaussctrl_amd.sd import ops
    c = lambda t: t.to(dt)
    vt, vtr = c(v).transpose(1, 2).contiguous(), c(vr).transpose(1, 2).contiguous()
    return ops.attention(c(qp), c(k), vt, heads, sets, f, Lk=k.shape[1], kref=c(kr), vtref=vtr, ref_fph=4, q_prescaled=True)


def _check_rows(got, qp, k, v, kr, vr, f, heads, dt, rows, sets=SETS, what="attention"):
    r = lambda t: t.to(dt).float()          # the reference sees the rounded operands the kernel multiplies
    ref = _ref_rows(r(qp), r(k), r(v), r(kr), r(vr), sets, f, heads, rows)
    sel = torch.gather(got, 1, rows[..., None].expand(-1, -1, got.shape[-1]))
    assert torch.isfinite(sel.float()).all(), what
    _close(sel, ref, dt, extra=8.0)         # P is rounded to the activation dtype before P V (as in the reference's fp16 bmm)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f,L,heads,D,kernel", [(6, 4096, 8, 40, "attn5"), (12, 4096, 8, 40, "attn5"), (12, 1024, 8, 80, "attn3"),
                                                (20, 1024, 8, 80, "attn3"), (12, 256, 8, 160, "wide+combine"), (20, 256, 8, 160, "wide+combine"),
                                                (12, 64, 8, 160, "attn+combine"), (20, 64, 8, 160, "attn+combine")])
def test_cross_view_attention_at_launch_set_batches(dt, f, L, heads, D, kernel, sel_log):
    """the product's cross-view attention (Q' prescaled, self set + 4 sets from the cached reference bank) at 12 / 24 / 40 CFG frames: k_attn5 in
    6 / 12 rounds of 256 workgroups, k_attn3 at D = 80, the set-split D = 160 forms; float64 on a seeded sample of query rows that touches every
    workgroup"""
    qp, k, v, kr, vr = _attn_inputs(f, L, heads, D, 10 + D)
    got = _run_attn(dt, qp, k, v, kr, vr, f, heads)
    assert _attns(sel_log) == [kernel]
    _check_rows(got, qp, k, v, kr, vr, f, heads, dt, _sample_rows(2 * f, L, 7))


# ------------------------------------------------------------------------------------------------------------- f16 / bf16 numerics edges

EDGE = [(2, 4096, 8, 40, "attn5", 256), (2, 1024, 8, 80, "attn3", 64)]      # (f, L, heads, D, kernel, queries per workgroup)


def _k5_sample_keys(L):
    """the keys k_attn5 (f16) samples for a set's exponent offset: key j (L / 64) + ((8 j + j / 8) mod (L / 64)), j < 64 (dn_attn5.hip)"""
    nt = L // 64
    return {j * nt + ((8 * j + (j >> 3)) % nt) for j in range(64)}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f,L,heads,D,kernel,qblk", EDGE)
def test_attention_overflow_in_one_bank_set(dt, f, L, heads, D, kernel, qblk, sel_log):
    """one key of reference set 2 (set 4 of 5, from the cached bank) beats its set's offset by ~50 binades for three query rows in three
    workgroups (both CFG halves): in f16 those workgroups leave the pipelined loop in the middle of the set loop for the safe body.  Every row
    stays within the bar, and every workgroup that holds none of those rows is bit-equal to the run without the spike."""
    h0, d0 = 3, 7
    col = h0 * D + d0
    qp, k, v, kr, vr = _attn_inputs(f, L, heads, D, 30 + D)
    qp[:, :, col] = 0.0                      # no other query sees channel d0 of head h0: the spike changes nothing else
    targets = [(1, 300 % L), (0, L - 5), (f + 1, (L // 2 + 17) % L)]
    for b, i in targets:
        qp[b, i, col] = 2.0
    ks = 2001 if L == 4096 else 700          # neither a k_attn5 sample key nor in the first key tile (k_attn3's offset)
    assert ks not in _k5_sample_keys(L) and ks >= 64
    clean = _run_attn(dt, qp, k, v, kr, vr, f, heads)
    krs = kr.clone()
    krs[[2, 6], ks, col] += 25.0             # bank rows of reference 2 in both halves
    got = _run_attn(dt, qp, k, v, kr=krs, vr=vr, f=f, heads=heads)
    assert _attns(sel_log) == [kernel, kernel]
    assert torch.isfinite(got.float()).all()
    rows = torch.cat([_sample_rows(2 * f, L, 8), torch.zeros(2 * f, 1, dtype=torch.long, device=DEV)], 1)
    for b, i in targets:
        rows[b, -1] = i
    _check_rows(got, qp, k, v, krs, vr, f, heads, dt, rows)
    same = torch.ones(2 * f, L, heads, dtype=torch.bool, device=DEV)
    for b, i in targets:
        same[b, (i // qblk) * qblk:(i // qblk + 1) * qblk, h0] = False
    g4, c4 = got.view(2 * f, L, heads, D), clean.view(2 * f, L, heads, D)
    assert torch.equal(g4[same], c4[same])
    for b, i in targets:                    # (and the spike did matter where it should)
        assert not torch.equal(g4[b, i, h0], c4[b, i, h0])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f,L,heads,D,kernel,qblk", EDGE)
def test_attention_logit_spread_sweep(dt, f, L, heads, D, kernel, qblk, sel_log):
    """Q' and K drawn at scale s (logits q'.k in binades, std s^2 sqrt(D)) for s = 0.25 .. 1.0 as in profiles/r06_attn5_f16_vs_bf16_spread.txt:
    from flat softmax rows to rows where f16's P range forces the safe body -- every point within the attention bar of float64"""
    for i, s in enumerate((0.25, 0.5, 0.75, 1.0)):
        qp, k, v, kr, vr = _attn_inputs(f, L, heads, D, 50 + i, qscale=s, kscale=s)
        got = _run_attn(dt, qp, k, v, kr, vr, f, heads)
        _check_rows(got, qp, k, v, kr, vr, f, heads, dt, _sample_rows(2 * f, L, 9 + i), what=f"qscale {s}")
    assert _attns(sel_log) == [kernel] * 4


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("f,L,heads,D,kernel,qblk", EDGE)
def test_attention_keys_far_below_the_sampled_maximum(dt, f, L, heads, D, kernel, qblk, sel_log):
    """a row with one dominant key at a position the offset is taken from (a k_attn5 sample key; k_attn3: the first key tile) and every other key
    of its own set 14 - 16 binades below it: P = 2^-14 .. 2^-16 is an f16 subnormal, and those keys carry ~12 % (L = 4096) / ~3 % (L = 1024) of the
    set's mass.  Flushing them to zero would move the row by several times the bar; the reference keeps them."""
    h0, d0 = 5, 11
    col = h0 * D + d0
    qp, k, v, kr, vr = _attn_inputs(f, L, heads, D, 70 + D)
    qp[:, :, col] = 0.0
    targets = [(0, 100 % L), (1, L - 1), (f, L // 3)]
    dom = 657 if L == 4096 else 5
    assert L != 4096 or dom in _k5_sample_keys(L)
    g = torch.Generator().manual_seed(12)
    for b, i in targets:
        qp[b, i, h0 * D:(h0 + 1) * D] = 0.0
        qp[b, i, col] = 1.0                  # logit of key j = K[b, j, col] exactly (binades)
        k[b, :, col] = (-14.0 - 2.0 * torch.rand(L, generator=g)).to(DEV)
        k[b, dom, col] = 0.0
    got = _run_attn(dt, qp, k, v, kr, vr, f, heads)
    assert _attns(sel_log) == [kernel]
    rows = torch.cat([_sample_rows(2 * f, L, 10), torch.zeros(2 * f, 1, dtype=torch.long, device=DEV)], 1)
    for b, i in targets:
        rows[b, -1] = i
    _check_rows(got, qp, k, v, kr, vr, f, heads, dt, rows)
    # the mass in question is real: without the floor keys the target rows would miss the bar by far
    r = lambda t: t.to(dt).float()
    for b, i in targets:
        kd = r(k[b]).double().view(L, heads, D)[:, h0]
        qd = r(qp[b, i]).double().view(heads, D)[h0]
        p = torch.softmax(kd @ qd * LN2, 0)
        assert float(1 - p[dom]) > 0.02
