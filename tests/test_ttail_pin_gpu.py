"""k_ttail / k_thead (csrc/dn_ttail.hip, csrc/dn_thead.hip) pinned per stage and per element to the float64 mirror of tests/_ttail_ref.py, through
the product library only: ops.transformer_tail / ops.transformer_head on weights.prepare of crafted state dicts.

Every case, its neutral weights and its bar are described in tests/_ttail_ref.py (CASES); tests/test_ttail_ref_cpu.py shows on the CPU that a
float32 oracle of the same function stays inside each bar and that each of eleven injected faults leaves one by a factor >= 18.  The reference
of a case is the mirror's value of the stage under test before its own rounding, every earlier stage rounded where the kernel packs.

Chain bars (all weights random; H4): `extra` = CHAIN_BAR = 2 E rounded up, E = CHAIN_E the smallest extra at which the oracle passes against
the mirror over all chain cases -- bf16: E = 7.9 -> 16, f16: E = 10.2 -> 21 (constants and measurement in tests/_ttail_ref.py)."""
import ctypes

import pytest
import torch

import _ttail_ref as R
from _margins import within
from _redzone import on_device
from _ttail_ref import C, CASES, BY_NAME, DTS, H, P
from test_denoise_kernels_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_prepared = {}                                     # the last (sd_key, dtype) only: consecutive cases share a state dict


def _w(m, dtype):
    from gaussctrl_amd.sd import weights
    key = (m["sd_key"], dtype)
    if key not in _prepared:
        _prepared.clear()
        _prepared[key] = weights.prepare(m["sd"], dtype, DEV, heads=H)
    return _prepared[key]


def _tail(m, dtype, w, **kw):
    from gaussctrl_amd.sd import ops, weights
    o1, h, x, k, vt = (on_device(m[n], DEV) for n in ("o1", "h", "x", "k", "vt"))
    kv = weights.tail_text_stream(k, vt, m["Lt"], H)
    kw.setdefault("halves", m["halves"])
    return ops.transformer_tail(o1, h, x, w[P + ".tail.a"], kv, w[P + ".tail.b"], w[P + ".tail.params"], H, kw.pop("f", m["f"]), m["Lt"], **kw)


def _head(m, dtype, w):
    from gaussctrl_amd.sd import ops
    h, qk, vt = ops.transformer_head(on_device(m["x"], DEV), on_device(m["coef"], DEV), w[P + ".head.w"], w[P + ".head.params"])
    return {"h": h, "q": qk[..., :C], "k": qk[..., C:], "vt": vt}


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case(name, dtype):
    case = BY_NAME[name]
    m = case.make(dtype)
    w = _w(m, dtype)
    got = {"out": _tail(m, dtype, w)} if case.kind == "tail" else _head(m, dtype, w)
    got = {k_: v.double().cpu() for k_, v in got.items()}
    ref = R.reference(m, case.kind, dtype)
    for label, s in R.shares(m, got, ref, dtype).items():
        print(f"{name} {label}: share of the bar {s:.4f}")
    extra = R.CHAIN_BAR[dtype] if m["extra"] == "chain" else m["extra"]
    for label, (out, rows) in m["groups"].items():
        g_, r_ = got[out], ref[out]
        if rows is not None:
            g_, r_ = (g_[:, :, rows], r_[:, :, rows]) if out == "vt" else (g_[:, rows], r_[:, rows])
        if m["add"] is None:
            _close(g_, r_, dtype, extra=extra)
        else:                                      # T5, H1: one output rounding + the absolute term of their fp32 arithmetic, no accumulation slack
            within(f"{label}: err / (one rounding + fp32 term)", R.share(g_, r_, dtype, extra, m["add"], slack=False), 1.0)
    if name.startswith("T5"):                      # the table against its own stated bound (dn_ttail.hip): |interpolated - gelu| <= 8.6e-6, per unit of hid
        hid = m["sd"][R.T + ".ff.net.0.proj.bias"][:R.FFN].double()
        q = int(name[-1])
        d = ((got["out"] - ref["out"]).abs() - R.EPS[dtype] * ref["out"].abs()).clamp_min(0) / hid[C * q:C * (q + 1)].abs()
        within("T5: |error| beyond one rounding, per unit of hid, against the table's 8.6e-6 (+ fp32 terms)", float(d.max()), 8.6e-6 + 2.0 ** -22 * 60)


def _chain_inputs(dtype, B, HW, Lt, seed=5):
    g = torch.Generator().manual_seed(seed)
    o1, h, x = (torch.randn(B, HW, C, generator=g).to(dtype) for _ in range(3))
    k, vt = R.text(g, 2, Lt, dtype)
    return dict(o1=o1, h=h, x=x, k=k, vt=vt, Lt=Lt, halves=1, f=B, sd=R.rand_sd(0), sd_key="chain0.0")


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
def test_bit_equalities(dtype):
    """no tolerance: the CFG-shared prefix (halves = 2 / in_rows) against explicit duplicates, a one-half launch against the first half of a
    two-half launch, frames permuted inside a half, and 128 identical rows (no lane, hg half or wave position computes differently)"""
    f, HW, Lt = 3, 128, 77
    m = _chain_inputs(dtype, f, HW, Lt)
    w = _w(m, dtype)
    two = _tail(m, dtype, w, halves=2)                                                        # [2 f, HW, C] from f input frames
    dup = dict(m, **{n: m[n].repeat(2, 1, 1) for n in ("o1", "h", "x")})
    assert torch.equal(two, _tail(dup, dtype, w, halves=1, f=f))
    one = _tail(dict(m, k=m["k"][:1], vt=m["vt"][:1]), dtype, w, halves=1, f=f)              # one CFG half
    assert torch.equal(one, two[:f])
    perm = [2, 0, 1]
    pm = dict(m, k=m["k"][:1], vt=m["vt"][:1], **{n: m[n][perm] for n in ("o1", "h", "x")})
    assert torch.equal(_tail(pm, dtype, w, halves=1, f=f), one[perm])
    same = dict(m, k=m["k"][:1], vt=m["vt"][:1], **{n: m[n][1:2, 5:6].expand(1, HW, C).contiguous() for n in ("o1", "h", "x")})
    out = _tail(same, dtype, w, halves=1, f=1)
    assert torch.equal(out, out[:, :1].expand_as(out)) and torch.equal(out[0, 0], one[1, 5])
    # head
    g = torch.Generator().manual_seed(6)
    hm = dict(x=(torch.randn(1, 1, C, generator=g) * 1.5).expand(1, HW, C).contiguous().to(dtype), coef=R._coef(g, 1, "mild"))
    o = _head(hm, dtype, w)
    for n in ("h", "q", "k"):
        assert torch.equal(o[n], o[n][:, :1].expand_as(o[n])), n
    assert torch.equal(o["vt"], o["vt"][:, :, :1].expand_as(o["vt"]))
    assert torch.equal(o["vt"][0, :, 0], _head(dict(hm, x=hm["x"].repeat(2, 1, 1), coef=hm["coef"].repeat(2, 1, 1)), dtype, w)["vt"][1, :, HW - 1])


def _tail_desc(M, HW, f, Lt, in_rows, bufs, channels=C):
    from gaussctrl_amd.sd import ops
    d = ops.TailDesc()
    d.dtype = ops.DT[torch.bfloat16]; d.channels = channels; d.heads = H; d.M = M; d.rows_per_frame = HW; d.in_rows = in_rows
    d.frames_per_half = f; d.text_len = Lt; d.ln_eps = 1e-5
    d.attn_out = d.resid = d.x_in = bufs["x"].data_ptr(); d.out = bufs["out"].data_ptr()
    d.w_a = bufs["w"][P + ".tail.a"].data_ptr(); d.w_kv = bufs["kv"].data_ptr(); d.w_b = bufs["w"][P + ".tail.b"].data_ptr()
    d.params = bufs["w"][P + ".tail.params"].data_ptr()
    return d


def test_refusals():
    """shapes the kernels are not built for are refused by the entry points with their own message, before anything is launched"""
    from gaussctrl_amd import _lib as L
    from gaussctrl_amd._lib import GaussCtrlHipError
    from gaussctrl_amd.sd import ops, weights
    dt = torch.bfloat16
    m = _chain_inputs(dt, 2, 128, 8)
    w = _w(m, dt)
    kv = weights.tail_text_stream(m["k"].to(DEV), m["vt"].to(DEV), 8, H)
    t = lambda B, HW, Cc=C: torch.zeros(B, HW, Cc, dtype=dt, device=DEV)
    call = lambda x, f, Lt, **kw: ops.transformer_tail(x, x, x, w[P + ".tail.a"], kv, w[P + ".tail.b"], w[P + ".tail.params"], H, f, Lt, **kw)
    for Lt in (0, 97):
        with pytest.raises(GaussCtrlHipError, match="text length <= 96"):
            call(t(2, 128), 1, Lt)
    for HW in (64, 192):
        with pytest.raises(GaussCtrlHipError, match="rows_per_frame must be a multiple of 128 dividing M"):
            call(t(2, HW), 1, 8)
        with pytest.raises(GaussCtrlHipError, match="rows_per_frame must be a multiple of 128 dividing M"):
            ops.transformer_head(t(2, HW), torch.zeros(2, C, 2, device=DEV), w[P + ".head.w"], w[P + ".head.params"])
    with pytest.raises(GaussCtrlHipError, match="the fused tail is built for C = 320"):
        call(t(2, 128, 256), 1, 8)
    with pytest.raises(GaussCtrlHipError, match="the fused head is built for C = 320"):
        ops.transformer_head(t(2, 128, 256), torch.zeros(2, 256, 2, device=DEV), w[P + ".head.w"], w[P + ".head.params"])
    with pytest.raises(GaussCtrlHipError, match="at most two CFG halves"):
        call(t(3, 128), 1, 8)
    # a CFG-shared launch whose in_rows does not divide M (3 frames of 128 rows, in_rows = 256): only the descriptor can say that
    bufs = dict(x=t(3, 128), out=t(3, 128), w=w, kv=kv)
    d = _tail_desc(3 * 128, 128, 3, 8, 256, bufs)
    with pytest.raises(GaussCtrlHipError, match="in_rows must be 0 or a multiple of 128 dividing M"):
        L.call("gc_dn_transformer_tail", ctypes.addressof(d))
    d = _tail_desc(3 * 128, 128, 3, 8, 64, bufs)
    with pytest.raises(GaussCtrlHipError, match="in_rows must be 0 or a multiple of 128 dividing M"):
        L.call("gc_dn_transformer_tail", ctypes.addressof(d))
