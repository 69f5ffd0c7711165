"""GPU: every selectable form of the head-size-40 cross-view attention (GC_ATTN_VAR_K4, K4_8WAVE, K4_Q64, D40_K3, RING4, RING8 and the default)
on the smallest shapes that reach every branch of the kernels' prologues (per-set K / V^T base addresses and the lane-parked table of them,
the offset-kernel LDS image, the DMA cursor with its ragged tail, the Q fragment load) -- against the float64 reference and bar of
tests/test_denoise_kernels_gpu.py.  heads 2, D 40, 2 frames per CFG half (4 frames), a reference bank of 2 x 4 frames:
  L = 256, five sets   4 tiles x 5 sets, Lq % 256 == 0: k_attn5's static-slot loop, the non-ragged k_attn3 / k_attn4
  L = 197, five sets   Lk % 64 != 0 and Lk % 8 != 0: the ragged instantiations (masked key rows, V^T chunk re-read, q < Lq guards)
  L = 256, one set     the single-set fold
each with Q prescaled and not, and once with a spiked key that sends the workgroup of query 17 to the in-kernel fallback."""
import dataclasses
import functools

import pytest
import torch

from test_denoise_kernels_gpu import DTS, _close, _rand, _ref_attn

pytestmark = pytest.mark.gpu
HEADS, D, F, RFPH = 2, 40, 2, 4
LN2, LOG2E = 0.6931471805599453, 1.4426950408889634
FIVE = [(-1, 0.6)] + [(r, 0.1) for r in range(4)]
ONE = [(-1, 1.0)]
# form -> (gc_attn_desc.kernel_variant bit of gaussctrl_amd.sd.ops, kernel when k_attn5's tile shapes fit, kernel when they do not)
FORMS = {"default": (None, "attn5", "attn4"), "RING4": ("GC_ATTN_VAR_RING4", "attn5", "attn4"), "RING8": ("GC_ATTN_VAR_RING8", "attn5", "attn4"),
         "K4": ("GC_ATTN_VAR_K4", "attn4", "attn4"), "K4_8WAVE": ("GC_ATTN_VAR_K4_8WAVE", "attn4", "attn4"),
         "K4_Q64": ("GC_ATTN_VAR_K4_Q64", "attn4", "attn4"), "D40_K3": ("GC_ATTN_VAR_D40_K3", "attn3", "attn3")}
K4_FORMS = ("K4", "K4_8WAVE", "K4_Q64")


@functools.lru_cache(maxsize=None)
def _problem(dt, L, nsets, pre, spiked):
    """operands in dt and the float64 reference, made once per shape and shared by every form (nothing writes to them)"""
    B, C = 2 * F, HEADS * D
    q = _rand((B, L, C), dt, 1.0, 1); k = _rand((B, L, C), dt, 1.0, 2); v = _rand((B, L, C), dt, 1.0, 3)
    kr = _rand((2 * RFPH, L, C), dt, 1.0, 4); vr = _rand((2 * RFPH, L, C), dt, 1.0, 5)
    if spiked:
        k[:, 200, :] = q[:, 17, :] * 40.0     # logit of (query 17, key 200) ~ 250 >> the offset of its set: the workgroup must recompute
    scale = D ** -0.5
    if pre:
        q = (q.float() * (scale * LOG2E)).to(dt)
        scale = LN2
    sets = FIVE if nsets == 5 else ONE
    bank = torch.arange(B, device=q.device) // F * RFPH
    ref = 0
    for kind, w in sets:
        kk, vv = (k, v) if kind == -1 else (kr[bank + kind], vr[bank + kind])
        ref = ref + w * _ref_attn(q, kk, vv, HEADS, scale)
    Lp = (L + 7) // 8 * 8

    def t(x):
        out = torch.zeros(x.shape[0], C, Lp, dtype=dt, device=x.device)
        out[:, :, :L] = x.transpose(1, 2)
        return out
    return q, k, t(v), kr, t(vr), sets, ref


def _run_forms(dt, L, nsets, pre, spiked, monkeypatch):
    from gaussctrl_amd.sd import ops
    q, k, vt, kr, vtr, sets, ref = _problem(dt, L, nsets, pre, spiked)
    fits5 = L % 64 == 0 and L % 256 == 0
    out = {}
    for name, (bit, k5, other) in FORMS.items():
        log = []
        monkeypatch.setattr(ops, "SELECTION_LOG", log)
        monkeypatch.setattr(ops, "OPTIONS", dataclasses.replace(ops.OPTIONS, attn_variant=getattr(ops, bit) if bit else 0))
        got = ops.attention(q, k, vt, HEADS, sets, F, Lk=L, kref=kr, vtref=vtr, ref_fph=RFPH, q_prescaled=pre)
        assert [s for kind, _, s in log if kind == "attn"] == [k5 if fits5 else other], name
        assert torch.isfinite(got.float()).all(), name
        _close(got, ref, dt, extra=8.0)      # P is rounded to the activation dtype before P V (as in the reference's fp16 bmm)
        out[name] = got
    return out


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("L,nsets", [(256, 5), (197, 5), (256, 1)])
def test_attention_forms(dt, L, nsets, pre, monkeypatch):
    """every form on its expected kernel, at the bar the default forms meet.  The three k_attn4 forms (4 waves, 8 waves, 64 queries per wave)
    give each wave its own queries and walk the same tile sequence: they agree bit for bit, as do the ring switches with the default."""
    out = _run_forms(dt, L, nsets, pre, False, monkeypatch)
    eq = {n: torch.equal(out[n], out["K4"]) for n in K4_FORMS}
    eq.update({n: torch.equal(out[n], out["default"]) for n in ("RING4", "RING8")})
    print(f"bit-equal (k_attn4 forms with K4, ring switches with the default), {dt}, L {L}, {nsets} sets, pre {pre}: {eq}")
    assert all(eq.values()), eq


@pytest.mark.parametrize("dt", DTS)
def test_attention_forms_offset_overflow(dt, monkeypatch):
    """the spiked key of test_attention_offset_overflow_falls_back in the own-frame set of the five: the workgroup that holds query 17 leaves for
    the online-softmax body, which runs on the LDS the offset kernel laid out.  (No bit-equality among the k_attn4 forms here: the fallback is
    taken per workgroup, and the forms' workgroups hold 128 or 256 queries.)"""
    _run_forms(dt, 256, 5, False, True, monkeypatch)
