"""The float64 mirror of the fused transformer head / tail (tests/_ttail_ref.py) checked on the CPU: it is the function the torch restatements
of tests/test_ttail_gpu.py state; its float32 oracle stays inside every bar of tests/test_ttail_pin_gpu.py on every case; and every injected
fault leaves the bar of at least one named case by a factor >= 2 (printed, with whether the old whole-output bar would have let it pass)."""
import functools
import math

import pytest
import torch

import _ttail_ref as R
from _ttail_ref import C, CASES, BY_NAME, DTS


@functools.lru_cache(maxsize=None)
def _made(name, dtype):
    return BY_NAME[name].make(dtype)


@functools.lru_cache(maxsize=None)
def _ref(name, dtype):
    return R.reference(_made(name, dtype), BY_NAME[name].kind, dtype)


def _oracle(name, dtype, mut=()):
    return R.outputs(_made(name, dtype), BY_NAME[name].kind, dtype, mut=mut)


def test_mirror_without_rounding_is_the_torch_restatement():
    """rnd=False: no rounding of weights or intermediates -> _torch_tail / _torch_head of tests/test_ttail_gpu.py to float32 accuracy"""
    import test_ttail_gpu as G
    sd = G._sd()
    g = torch.Generator().manual_seed(1)
    B, HW, f, Lt = 4, 128, 2, 50
    o1, h, x = (torch.randn(B, HW, C, generator=g).bfloat16() for _ in range(3))
    ctx = torch.randn(B // f, Lt, G.CTX, generator=g).bfloat16()
    ref = G._torch_tail(sd, o1, h, x, ctx, f)
    k = ctx.double() @ sd[G.T + ".attn2.to_k.weight"].double().T
    vt = (ctx.double() @ sd[G.T + ".attn2.to_v.weight"].double().T).transpose(1, 2)
    got = R.tail(sd, o1, h, x, k, vt, f, Lt, torch.bfloat16, rnd=False)
    assert float((got - ref.double()).abs().max() / ref.abs().max()) < 2e-5
    # head: GroupNorm coefficients from the statistics in float64
    sd[G.P + ".norm.weight"] = 1 + 0.1 * torch.randn(C, generator=g); sd[G.P + ".norm.bias"] = 0.1 * torch.randn(C, generator=g)
    xh = (torch.randn(2, 128, C, generator=g) * 1.5 + 0.3).bfloat16()
    xg = xh.double().view(2, 128, 32, 10)
    mean = xg.mean((1, 3)); rstd = torch.rsqrt(xg.var((1, 3), unbiased=False) + 1e-6)
    a = rstd.repeat_interleave(10, 1) * sd[G.P + ".norm.weight"].double()
    d = sd[G.P + ".norm.bias"].double() - mean.repeat_interleave(10, 1) * a
    outs = R.head(sd, xh, torch.stack([a, d], -1), torch.bfloat16, rnd=False)
    for name, t in zip(("h", "q", "k", "vt"), G._torch_head(sd, xh)):
        assert float((outs[name] - t.double()).abs().max() / t.abs().max()) < 2e-5, name


def test_share_is_close_of_the_denoise_kernel_tests():
    """share() <= 1 exactly when _close of tests/test_denoise_kernels_gpu.py passes"""
    from _margins import RECORDS
    from test_denoise_kernels_gpu import _close
    n_rec = len(RECORDS)
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(64, 64, generator=g, dtype=torch.float64)
    for dt in DTS:
        for k_, ok in ((0.9, True), (1.2, False)):
            got = ref + k_ * R.EPS[dt] * 2.0 * (ref.abs() + 0.05 * ref.abs().max())
            assert (R.share(got, ref, dt, 2.0) <= 1.0) == ok
            try:
                _close(got, ref, dt, extra=2.0); passed = True
            except AssertionError:
                passed = False
            assert passed == ok
    del RECORDS[n_rec:]                            # (the deliberate failures are no margins of the suite)


def test_gelu_table_returns_8_at_gate_8():
    """T2 relies on it: gate = 8 is the clamped last segment with fraction 1, and e.x + 1 * e.y is exactly 8 in fp32"""
    from gaussctrl_amd.sd import weights
    tab = weights.gelu_table("cpu").reshape(-1, 2)
    t = torch.tensor(8.0 * weights.GELU_STEP + 0.5 * weights.GELU_N)
    ti = t.clamp(0, weights.GELU_N - 1).floor()
    e = tab[int(ti)]
    assert float(torch.addcmul(e[0], t - ti, e[1])) == 8.0 and float(t - ti) == 1.0


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
def test_chain_bar_is_twice_the_oracle_s_own_error(dtype):
    """E = the smallest `extra` at which the float32 oracle passes against the mirror over all chain cases (tail chains and H4)"""
    E, worst = 0.0, None
    for c in CASES:
        m = _made(c.name, dtype)
        if m["extra"] != "chain":
            continue
        ref, got = _ref(c.name, dtype), _oracle(c.name, dtype)
        for label, (name, _) in m["groups"].items():
            e = R.needed_extra(got[name], ref[name], dtype)
            if e > E:
                E, worst = e, f"{c.name}.{label}"
    print(f"E({dtype}) = {E:.3f} at {worst}; constants: E = {R.CHAIN_E[dtype]}, bar = {R.CHAIN_BAR[dtype]}")
    assert E <= R.CHAIN_E[dtype] <= 2 * E, E
    assert R.CHAIN_BAR[dtype] == math.ceil(2 * R.CHAIN_E[dtype])


@pytest.mark.parametrize("dtype", DTS, ids=["bf16", "f16"])
def test_oracle_is_inside_every_bar(dtype):
    worst = {}
    for c in CASES:
        for label, s in R.shares(_made(c.name, dtype), _oracle(c.name, dtype), _ref(c.name, dtype), dtype).items():
            assert s <= 1.0, (c.name, label, s)
            fam = c.name.split("-")[0]
            worst[fam] = max(worst.get(fam, 0.0), s)
    print({k_: round(v, 3) for k_, v in worst.items()})


# the named cases each injected fault is looked for in
MUT_CASES = {
    "mask_last": ["T3-onehot-Lt33", "T3-onehot-Lt96", "T3-ordinary-Lt7", "T3-low-Lt1"],
    "text_half0": ["T3-ordinary-Lt77", "T3-onehot-Lt32"],
    "bo2_hole": ["T4"],
    "bup_hole": ["T5-set0-q1"],
    "gelu_shift": [f"T5-set{s}-q0" for s in range(5)],
    "gelu_tanh": [f"T5-set{s}-q0" for s in range(5)],
    "res_h1": ["T4", "chain-B2f1HW128-Lt77"],
    "ln_319": ["T2-A", "H3-A"],
    "ln_eps": ["T2-A", "H3-A"],
    "gn_img0": ["H1", "H4-HW128"],
    "vt_q": ["H4-HW128", "H4-HW256"],
}


def _old_bar_lets_it_pass(mut, dtype):
    """the mutated oracle under the bars of tests/test_ttail_gpu.py (fp32 unrounded reference, max-norm over the whole output: below
    2e-2 / 3e-3 of max|ref| AND below 2 x the unmutated path's error + 1e-3), at that file's random weights and a two-half shape"""
    bar = 2e-2 if dtype == torch.bfloat16 else 3e-3
    if mut in ("gn_img0", "vt_q"):
        m = _made("H4-HW128", dtype)
        run = lambda **kw: R.head(m["sd"], m["x"], m["coef"], dtype, **kw)
        names = ("h", "q", "k", "vt")
    else:
        m = _made("chain-B4f2HW256-Lt77", dtype)
        run = lambda **kw: {"out": R.tail(m["sd"], m["o1"], m["h"], m["x"], m["k"], m["vt"], m["f"], m["Lt"], dtype, **kw)}
        names = ("out",)
    ref, base, got = run(rnd=False), run(acc=torch.float32), run(acc=torch.float32, mut=(mut,))
    ok = True
    for n in names:
        sc = ref[n].abs().max()
        e, e0 = float((got[n] - ref[n]).abs().max() / sc), float((base[n] - ref[n]).abs().max() / sc)
        ok = ok and e < bar and e < 2 * e0 + 1e-3
    return ok


def test_every_mutation_leaves_a_bar_by_a_factor_of_two():
    assert set(MUT_CASES) == set(R.MUTATIONS)
    least = float("inf")
    for mut, names in MUT_CASES.items():
        for dtype in DTS:
            best, where = 0.0, None
            for name in names:
                if mut in R.HEAD_MUTATIONS[:2] and BY_NAME[name].kind != "head":
                    continue
                got = _oracle(name, dtype, mut=(mut,))
                for label, s in R.shares(_made(name, dtype), got, _ref(name, dtype), dtype).items():
                    s = float("inf") if s != s else s                      # NaN (e.g. l = 0): no bar admits it
                    if s > best:
                        best, where = s, f"{name}.{label}"
            old = _old_bar_lets_it_pass(mut, dtype)
            print(f"{mut:11s} {str(dtype)[6:]:8s} x{best:<10.3g} beyond the bar at {where}; old whole-output bar lets it pass: {old}")
            assert best >= 2.0, (mut, dtype, best)
            least = min(least, best)
    print(f"least factor over the list: x{least:.3g}")
