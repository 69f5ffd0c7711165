"""Float64 mirror of the two fused transformer kernels (csrc/dn_ttail.hip k_ttail, csrc/dn_thead.hip k_thead), a float32 oracle of the same
function with mutation hooks, and the crafted cases the CPU and GPU tests share (tests/test_ttail_ref_cpu.py, tests/test_ttail_pin_gpu.py).

ROUNDING POINTS.  The mirror takes exactly the 16-bit tensors the kernel receives and rounds, R(.) = .to(dtype), exactly where the kernel
packs its registers.  pack2<T> / pack8<T> (csrc/dn_common.h) convert a float pair with __builtin_convertvector to __bf16 / _Float16, i.e.
v_cvt_pk_bf16_f32 / v_cvt_f16_f32 in the default rounding mode: round to nearest even, overflow to infinity, 16-bit
subnormals kept -- what torch's .to(dtype) does.  Weights are rounded once from the fp32 masters, with D^-1/2 log2(e) folded into both
to_q weights in fp32 BEFORE that rounding (weights.prepare); biases and norm affines stay fp32; the text K [halves, Lt, 320] and V^T
[halves, 320, >= Lt] are the 16-bit tensors handed to weights.tail_text_stream.

  tail, per row:   h1 = R(o1 Wo1^T + bo1 + h)      n2 = R(LN(h1; g2, b2))     q2 = R(n2 Wq2'^T)
                   per head: s = q2_h K_h^T over keys < Lt,  p = R(2^(s - max s)),  l = sum of the ROUNDED p (the ones row of V^T),
                             o2 = R((sum p v) / l)
                   h2 = R(o2 Wo2^T + bo2 + h1)     n3 = R(LN(h2; g3, b3))     u = n3 Wup^T + bup  (NOT rounded)
                   ff = R(hid gelu(gate))  (exact erf GELU: the kernel's 2048-entry table is part of what is measured)
                   h3 = R(ff Wdn^T + bdn + h2)     out = R(h3 Wpo^T + bpo + x)
                   text half of a row = (row // HW) // frames_per_half; with halves = 2 (gc_ttail_desc.in_rows) output row m reads input
                   row m % in_rows
  head, per row:   xn = R(x a + d)  (coef [B, C, 2] fp32 handed in, image = row // HW)       h = R(xn Win^T + bin)
                   n1 = R(LN(h; g1, b1))           q = R(n1 Wq'^T)   k = R(n1 Wk^T)   vt = R(Wv n1^T)

ORACLE.  acc=torch.float32 runs the same function with float32 accumulation in another order (k summed in chunks of 16, as the MFMAs
consume it): an independent draw of the summation-order noise the kernel has.  `mut` names faults injected into it (MUTATIONS).

ISOLATION.  With W = I and zero bias a projection is exact in the MFMA (one nonzero product per output, fp32 accumulate); with W = 0 and zero
bias a stage hands its residual on unchanged.  The cases below set all stages but one neutral, so that one stage's output is `out` bit for
bit.  The two LayerNorms of the tail: LN2 is held through the text attention (T3: Wq2' = I, q2 = n2); LN3 through the feed-forward (T2: the
hidden half of the up-projection is a 320-column identity / 8, every gate is the bias 8 where the table returns exactly 8, the down
projection selects): out = R(n3 + h2).  The residual cannot be taken out of that sum, so the LN3 rows use a gamma / an input scale at which n3
is not small against h2 -- except the rows near the largest finite f16, which show overflow and gross error only; LayerNorm1 of the head
(H3: q = k = vt^T = n1 bit for bit) carries every row class undiluted, through the same code.

BARS (share()): tests/test_denoise_kernels_gpu.py::_close -- one output rounding EPS |ref|, times `extra`, plus 5 % of it at max|ref|, plus
1e-6; no element exempt.  `extra` of an isolated stage is what its per-op twin has there (linear 1, LayerNorm 2, attention 8); T5 and H1
take one rounding plus an absolute term (their fp32 arithmetic); the chain bar is 2 E, E measured oracle-against-mirror (CHAIN_E)."""
import math

import torch

C, H, D, FFN, T = 320, 8, 40, 1280, "tb.transformer_blocks.0"
P = "tb"
LOG2E = 1.4426950408889634
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
DTS = [torch.bfloat16, torch.float16]

MUTATIONS = ["mask_last", "text_half0", "bo2_hole", "bup_hole", "gelu_shift", "gelu_tanh", "res_h1", "ln_319", "ln_eps", "gn_img0", "vt_q"]
HEAD_MUTATIONS = ("gn_img0", "vt_q", "ln_319", "ln_eps")


# ------------------------------------------------------------------------------------------------------------------ the function
def _mm(x, w, acc, init=None):
    """x [M, K] w [N, K]^T (+ init): float64 at once; float32 in k-chunks of 16 on top of the initial value (bias + residual first, like
    the kernel's accumulators)"""
    if acc == torch.float64:
        y = x @ w.T
        return y if init is None else y + init
    y = torch.zeros(x.shape[0], w.shape[0], dtype=acc) if init is None else init.clone()
    for c in range(0, x.shape[1], 16):
        y = y + x[:, c:c + 16] @ w[:, c:c + 16].T
    return y


def _ln(x, g, b, eps, mut):
    n = 319.0 if "ln_319" in mut else 320.0
    eps = 1e-6 if "ln_eps" in mut else eps
    mean = x.sum(-1, keepdim=True) / 320.0
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / n
    return d * torch.rsqrt(var + eps) * g + b


def gelu(x, mut=()):
    if "gelu_shift" in mut:
        x = x + 1.0 / 128
    if "gelu_tanh" in mut:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))         # (erfc: no cancellation at negative gates)


def _weights(sd, names, dtype, acc, rnd):
    """fp32 masters -> (scale folded into to_q) -> ONE rounding to dtype -> acc; vectors stay fp32 -> acc"""
    out = {}
    for key, name in names.items():
        v = sd[name].float()
        if v.dim() == 1:
            out[key] = v.to(acc)
            continue
        v = v.reshape(v.shape[0], -1)
        if name.endswith(".to_q.weight"):
            v = v * (D ** -0.5 * LOG2E) if rnd else v.double() * (D ** -0.5 * LOG2E)
        out[key] = (v.to(dtype) if rnd else v).to(acc)
    return out


TAIL_NAMES = {"wo1": T + ".attn1.to_out.0.weight", "bo1": T + ".attn1.to_out.0.bias", "g2": T + ".norm2.weight", "b2": T + ".norm2.bias",
              "wq2": T + ".attn2.to_q.weight", "wo2": T + ".attn2.to_out.0.weight", "bo2": T + ".attn2.to_out.0.bias",
              "g3": T + ".norm3.weight", "b3": T + ".norm3.bias", "wup": T + ".ff.net.0.proj.weight", "bup": T + ".ff.net.0.proj.bias",
              "wdn": T + ".ff.net.2.weight", "bdn": T + ".ff.net.2.bias", "wpo": P + ".proj_out.weight", "bpo": P + ".proj_out.bias"}
HEAD_NAMES = {"win": P + ".proj_in.weight", "bin": P + ".proj_in.bias", "g1": T + ".norm1.weight", "b1": T + ".norm1.bias",
              "wq": T + ".attn1.to_q.weight", "wk": T + ".attn1.to_k.weight", "wv": T + ".attn1.to_v.weight"}


def tail(sd, o1, h, x, k, vt, f, Lt, dtype, acc=torch.float64, rnd=True, mut=(), halves=1, eps=1e-5, taps=None):
    """o1, h, x [B, HW, 320]; k [nh, >= Lt, 320], vt [nh, 320, >= Lt] -> out [halves B, HW, 320] in `acc`.  taps: a dict that receives every
    stage's value BEFORE its rounding ([rows, 320]; the flow itself goes on with the rounded value)"""
    taps = {} if taps is None else taps

    def R(v, name=None):
        if name:
            taps[name] = v
        return v.to(dtype).to(acc) if rnd else v
    w = _weights(sd, TAIL_NAMES, dtype, acc, rnd)
    if halves > 1:                                                     # in_rows: output row m reads input row m % in_rows
        o1, h, x = (t.repeat(halves, 1, 1) for t in (o1, h, x))
    B, HW, _ = o1.shape
    o1, h, x = (t.to(acc).reshape(B * HW, C) for t in (o1, h, x))
    k, vt = k.to(acc), vt.to(acc)
    h1 = R(_mm(o1, w["wo1"], acc, w["bo1"] + h), "h1")
    n2 = R(_ln(h1, w["g2"], w["b2"], eps, mut), "n2")
    q2 = R(_mm(n2, w["wq2"], acc)).view(B * HW, H, D)
    half = torch.zeros(B * HW, dtype=torch.long) if "text_half0" in mut else (torch.arange(B * HW) // HW) // f
    assert int(half.max()) < k.shape[0]
    nk = Lt - 1 if "mask_last" in mut and Lt > 1 else Lt
    o2, o2raw = torch.zeros(B * HW, H, D, dtype=acc), torch.zeros(B * HW, H, D, dtype=acc)
    for hf in range(k.shape[0]):
        rows = half == hf
        if not bool(rows.any()):
            continue
        s = torch.einsum("mhd,jhd->mhj", q2[rows], k[hf, :nk].reshape(nk, H, D))
        p = R(torch.exp2(s - s.amax(-1, keepdim=True)))
        o2raw[rows] = torch.einsum("mhj,hdj->mhd", p, vt[hf, :, :nk].reshape(H, D, nk)) / p.sum(-1, keepdim=True)
        o2[rows] = R(o2raw[rows])
    taps["o2"] = o2raw.reshape(B * HW, C)
    bo2 = w["bo2"].clone()
    if "bo2_hole" in mut:
        bo2[288:] = 0
    h2 = R(_mm(o2.reshape(B * HW, C), w["wo2"], acc, bo2 + h1), "h2")
    n3 = R(_ln(h2, w["g3"], w["b3"], eps, mut), "n3")
    bup = w["bup"].clone()
    if "bup_hole" in mut:                                              # one 64-channel feed-forward iteration (it = 7) without its bias
        bup[448:512] = 0; bup[FFN + 448:FFN + 512] = 0
    u = _mm(n3, w["wup"], acc, bup.expand(B * HW, -1))
    ff = R(u[:, :FFN] * gelu(u[:, FFN:], mut), "ff")
    h3 = R(_mm(ff, w["wdn"], acc, w["bdn"] + (h1 if "res_h1" in mut else h2)))
    return R(_mm(h3, w["wpo"], acc, w["bpo"] + x), "out").view(B, HW, C)


def head(sd, x, coef, dtype, acc=torch.float64, rnd=True, mut=(), eps=1e-5, taps=None):
    """x [B, HW, 320], coef [B, 320, 2] fp32 -> h [B, HW, 320], q, k [B, HW, 320], vt [B, 320, HW] in `acc`; taps as in tail ([B, HW, 320] each)"""
    taps = {} if taps is None else taps
    B, HW, _ = x.shape

    def R(v, name=None):
        if name:
            taps[name] = v.reshape(B, HW, C)
        return v.to(dtype).to(acc) if rnd else v
    w = _weights(sd, HEAD_NAMES, dtype, acc, rnd)
    cf = coef.to(acc)
    if "gn_img0" in mut:
        cf = cf[:1].expand(B, -1, -1)
    xn = R(x.to(acc) * cf[:, None, :, 0] + cf[:, None, :, 1], "xn").reshape(B * HW, C)
    hh = R(_mm(xn, w["win"], acc, w["bin"].expand(B * HW, -1)), "h")
    n1 = R(_ln(hh, w["g1"], w["b1"], eps, mut), "n1")
    q, k = R(_mm(n1, w["wq"], acc), "q"), R(_mm(n1, w["wk"], acc), "k")
    v = R(_mm(n1, w["wq" if "vt_q" in mut else "wv"], acc), "v")
    return {"h": hh.view(B, HW, C), "q": q.view(B, HW, C), "k": k.view(B, HW, C), "vt": v.view(B, HW, C).transpose(1, 2).contiguous()}


# ------------------------------------------------------------------------------------------------------------------ the bar
def share(got, ref, dt, extra=1.0, add=None, slack=True):
    """max over ALL elements of |got - ref| / allowed; allowed = _close's (EPS extra |ref| + 5 % of that at max|ref| + 1e-6) when
    slack, else one rounding EPS |ref| plus the absolute term `add` (plus 2^-24: half a step of the smallest f16 subnormals).
    <= 1 passes.  NaN / inf anywhere gives NaN or inf, which no bar admits."""
    got, ref = got.double().cpu(), ref.double().cpu()
    tol = EPS[dt] * extra
    allowed = tol * ref.abs() + (tol * ref.abs().max() * 0.05 + 1e-6 if slack else 2.0 ** -24)
    if add is not None:
        allowed = allowed + add.double()
    r = (got - ref).abs() / allowed
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def needed_extra(got, ref, dt):
    """the smallest `extra` at which share(got, ref, dt, extra) <= 1"""
    got, ref = got.double(), ref.double()
    e = ((got - ref).abs() - 1e-6) / (EPS[dt] * (ref.abs() + 0.05 * ref.abs().max()))
    return max(float(e.max()), 0.0)


# ------------------------------------------------------------------------------------------------------------------ crafted state dicts
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def neutral_sd():
    """every projection 0 with zero bias except proj_out = I (out = h3), every LayerNorm gamma 1 / beta 0, proj_in = I: each stage hands its
    residual on, bit for bit"""
    z = torch.zeros
    sd = {P + ".proj_in.weight": torch.eye(C).reshape(C, C, 1, 1), P + ".proj_in.bias": z(C),
          P + ".proj_out.weight": torch.eye(C).reshape(C, C, 1, 1), P + ".proj_out.bias": z(C),
          T + ".ff.net.0.proj.weight": z(2 * FFN, C), T + ".ff.net.0.proj.bias": z(2 * FFN),
          T + ".ff.net.2.weight": z(C, FFN), T + ".ff.net.2.bias": z(C)}
    for n in ("norm1", "norm2", "norm3"):
        sd[T + f".{n}.weight"] = torch.ones(C); sd[T + f".{n}.bias"] = z(C)
    for a in ("attn1", "attn2"):
        for m in ("to_q", "to_k", "to_v", "to_out.0"):
            sd[T + f".{a}.{m}.weight"] = z(C, C)
        sd[T + f".{a}.to_out.0.bias"] = z(C)
    return sd


def scaled_eye():
    """to_q master whose folded, rounded weight is I (fp32 (1 / s) s rounds to 1 in 16 bits)"""
    return torch.eye(C) / (D ** -0.5 * LOG2E)


def rand_sd(seed=0, gate_shift=0.0):
    """all weights random: _sd() of tests/test_ttail_gpu.py"""
    from test_ttail_gpu import _sd
    return _sd(seed, gate_shift)


def _r(g, *s, sc=1.0):
    return torch.randn(*s, generator=g) * sc


def text(g, nh, Lt, dtype, k_scale=0.3):
    """text K [nh, Lt, 320] and V^T [nh, 320, Lp] (Lp = Lt rounded up to 8; the columns past Lt hold 777: never read)"""
    Lp = (Lt + 7) // 8 * 8
    k = _r(g, nh, Lt, C, sc=k_scale)
    vt = torch.full((nh, C, Lp), 777.0)
    vt[:, :, :Lt] = _r(g, nh, C, Lt)
    return k.to(dtype), vt.to(dtype)


# LayerNorm rows.  SIGN: the per-channel sign pattern of the "cancel" rows and of beta A.
SIGN = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
LN_A = (torch.ones(C), -SIGN * (127.0 / 128))                       # beta cancels a two-valued row's +-1: what is left is rstd's error, x 128


def ln_affine(which):
    """A: gamma 1, beta LN_A.  B / C: gamma ~ 4096 / ~ 256, beta ~ 64.  (T2 shows R(n3 + h2): where the two cancel, the rounding of n3 -- half a
    step at |h2| -- meets the 5 % accumulation slack of max|ref| alone, so on the rows at 1000 gamma makes max|n3| > 10240; on the rows near the
    largest finite f16 it keeps n3 + h2 finite)"""
    if which == "A":
        return LN_A
    g = _gen(41)
    return (4096.0 if which == "B" else 256.0) * (1 + 0.1 * _r(g, C)), 64.0 * _r(g, C)


def ln_rows(which, dtype):
    """[128, 320] rows and {class: row slice}.  A (gamma 1, beta LN_A): variance 0 (output = beta), variance ~ eps, variance ~ 1, and two-valued
    rows s_c a whose normalised value +-1 beta cancels to 1 / 128.  B: mean 1000 x std.  C: |values| near the largest finite f16, of both signs and of one.
    (Variance-0 rows stay below 4: the kernel's mean is sum * fl(1 / 320), one fp32 step off for some constants, and x - mean is then
    measured against eps = 1e-5 alone -- at a constant 1000 that is 0.02 gamma.)"""
    g = _gen(40)
    rows = torch.zeros(128, C)
    if which == "A":
        cls = {"var0": slice(0, 32), "var_eps": slice(32, 64), "var1": slice(64, 96), "cancel": slice(96, 128)}
        rows[0:32] = torch.tensor([0.0, 0.5, -2.0, 3.140625]).repeat(8)[:, None]
        rows[32:64] = 2.0 ** -6 + 0.003 * _r(g, 32, C)
        rows[64:96] = _r(g, 32, C)
        rows[96:128] = SIGN[None] * torch.tensor([2.0 ** -6, 2.0 ** -5, 2.0 ** -4, 1.0]).repeat(8)[:, None]
    elif which == "B":
        cls = {"mean1000": slice(0, 128)}
        rows[:] = 1000.0 + _r(g, 128, C)
    else:
        cls = {"near_max_signs": slice(0, 64), "near_max_pos": slice(64, 128)}
        sgn = torch.where(torch.rand(64, C, generator=g) < 0.5, -1.0, 1.0)
        rows[0:64] = sgn * (61000.0 + 1500.0 * torch.rand(64, C, generator=g))
        rows[64:128] = 62000.0 + 150.0 * _r(g, 64, C).clamp(-3, 3)
    return rows.to(dtype), cls


# T5: the gates.  knots i / 128 over [-9, 9], midpoints, the named edges, random offsets: 5 bias sets of 1280
def t5_gates():
    g = _gen(50)
    kn = torch.arange(-9 * 128, 9 * 128 + 1, dtype=torch.float64) / 128
    edge = torch.tensor([8.0, -8.0, 8 - 1 / 128, -(8 - 1 / 128), 8.5, -8.5, 14.0, -14.0, 60.0, -60.0, 0.0, -0.0, 1e-30, -1e-30])
    n = 5 * FFN - 2 * kn.numel() + 1 - edge.numel()
    rnd = (torch.rand(n, generator=g, dtype=torch.float64) * 18 - 9)
    gates = torch.cat([kn, kn[:-1] + 1 / 256, edge.double(), rnd]).float()
    gates = gates[torch.randperm(gates.numel(), generator=g)]
    hid = torch.where(torch.rand(gates.numel(), generator=g) < 0.5, 1.0, -3.5)
    return gates.reshape(5, FFN), hid.reshape(5, FFN)


class Case:
    """name; kind 'tail' | 'head'; make(dtype) -> dict(sd=, sd_key=, inputs..., groups={label: (output name, row slice or None)},
    extra= number | 'chain', add= optional absolute term per element (then no accumulation slack))"""

    def __init__(self, name, kind, make):
        self.name, self.kind, self.make = name, kind, make

    def __repr__(self):
        return self.name


def _tail_case(sd, sd_key, dtype, B, HW, f, Lt, seed, *, extra, ref, o1=None, h=None, x=None, kv=None, halves=1, groups=None, add=None, h_scale=1.0):
    g = _gen(seed)
    mk = lambda t, sc=1.0: (_r(g, B, HW, C, sc=sc) if t is None else t).to(dtype)
    o1, h, x = mk(o1), mk(h, h_scale), mk(x)
    nh = halves if halves > 1 else B // f
    k, vt = text(g, nh, Lt, dtype) if kv is None else kv
    return dict(sd=sd, sd_key=sd_key, o1=o1, h=h, x=x, k=k, vt=vt, f=f, Lt=Lt, halves=halves, extra=extra, add=add, ref=ref,
                groups=groups or {"out": ("out", None)})


def _t1(dtype):
    sd = neutral_sd(); g = _gen(11)
    sd[T + ".attn1.to_out.0.weight"] = _r(g, C, C, sc=C ** -0.5); sd[T + ".attn1.to_out.0.bias"] = _r(g, C, sc=0.1)
    return _tail_case(sd, "t1", dtype, 2, 128, 1, 77, 12, extra=1.0, ref=lambda t, c: t["h1"], x=torch.zeros(2, 128, C))


def _t2(which):
    def make(dtype):
        sd = neutral_sd()
        gam, bet = ln_affine(which)
        sd[T + ".norm3.weight"] = gam.clone(); sd[T + ".norm3.bias"] = bet.clone()
        sd[T + ".ff.net.0.proj.weight"][:C] = torch.eye(C) / 8         # hidden channels 0..319 = n3 / 8 (fp32, not rounded); every gate = its bias
        sd[T + ".ff.net.0.proj.bias"][FFN:] = 8.0                     # the table returns exactly 8 there (test_ttail_ref_cpu.py): ff = n3
        sd[T + ".ff.net.2.weight"][:, :C] = torch.eye(C)
        rows, cls = ln_rows(which, dtype)
        z = torch.zeros(1, 128, C)
        return _tail_case(sd, "t2" + which, dtype, 1, 128, 1, 7, 21, extra=2.0, ref=lambda t, c: t["n3"] + c["h"].double().reshape(-1, C), o1=z, h=rows[None], x=z,
                          groups={c: ("out", s) for c, s in cls.items()})
    return make


def _t3_sd():
    sd = neutral_sd()
    gam, bet = torch.ones(C), torch.zeros(C)
    gam[::D] = 0.0; bet[::D] = 8.0                                     # channel 0 of every head: q = 8 for every row
    sd[T + ".norm2.weight"] = gam; sd[T + ".norm2.bias"] = bet
    sd[T + ".attn2.to_q.weight"] = scaled_eye()                        # q2 = n2: LayerNorm2 is held here
    sd[T + ".attn2.to_out.0.weight"] = torch.eye(C)                    # h2 = R(o2 + h1), h1 = h = randn / 64
    return sd


def _t3(Lt, kind):
    def make(dtype):
        g = _gen(300 + Lt)
        k, vt = text(g, 2, Lt, dtype)                                  # distinct text per CFG half
        k = k.float()
        k[:, :, ::D] = 0.0                                             # logit = 8 k[j, head channel 0] + ordinary part (std ~ 1.9)
        if kind == "onehot":                                           # one logit 176 (base 2) above: P one-hot, the rest underflow to 0
            k[0, Lt - 1, ::D] = 22.0                                   # half 0: the LAST valid key
            k[1, Lt // 2, ::D] = 22.0
        if kind == "low":                                              # every valid logit ~ -160: only the mask keeps the maximum on a valid key
            k[:, :, ::D] = -20.0                                       # (the keys past Lt are zero rows of the stream: logit 0)
        return _tail_case(_t3_sd(), "t3", dtype, 2, 128, 1, Lt, 31, extra=8.0, ref=lambda t, c: t["o2"] + c["h"].double().reshape(-1, C), o1=torch.zeros(2, 128, C), x=torch.zeros(2, 128, C),
                          kv=(k.to(dtype), vt), h_scale=2.0 ** -6)
    return make


def _t4(dtype):
    """to_out2 on an exactly known o2: 40 one-hot keys per head (K = 24 e_j), rows whose LayerNorm2 output is sqrt(39) at channel
    j(row, head) = (row + 5 head) % 40 of every head and -1 / sqrt(39) elsewhere: the logit of key j is 153 above the rest, P is one-hot, l = 1
    and o2 = V[j] bit for bit, different from row to row"""
    sd = neutral_sd(); g = _gen(14)
    sd[T + ".attn2.to_q.weight"] = scaled_eye()
    sd[T + ".attn2.to_out.0.weight"] = _r(g, C, C, sc=C ** -0.5); sd[T + ".attn2.to_out.0.bias"] = _r(g, C, sc=0.1)
    B, HW, Lt = 2, 128, 40
    h = torch.zeros(B * HW, C)
    j = (torch.arange(B * HW)[:, None] + 5 * torch.arange(H)[None]) % D
    h[torch.arange(B * HW)[:, None], torch.arange(H)[None] * D + j] = 1.0
    k = torch.zeros(2, Lt, C)
    for hd in range(H):
        k[:, torch.arange(D), hd * D + torch.arange(D)] = 24.0
    _, vt = text(g, 2, Lt, dtype)
    z = torch.zeros(B, HW, C)
    return _tail_case(sd, "t4", dtype, B, HW, 1, Lt, 15, extra=1.0, ref=lambda t, c: t["h2"], o1=z, h=h.view(B, HW, C), x=z, kv=(k.to(dtype), vt))


def _t5(s, q):
    def make(dtype):
        gates, hid = t5_gates()
        sd = neutral_sd()
        sd[T + ".ff.net.0.proj.bias"] = torch.cat([hid[s], gates[s]])
        sel = torch.zeros(C, FFN); sel[torch.arange(C), torch.arange(C) + C * q] = 1.0
        sd[T + ".ff.net.2.weight"] = sel
        gq, hq = gates[s, C * q:C * (q + 1)].double(), hid[s, C * q:C * (q + 1)].double()
        add = hq.abs() * (8.6e-6 + 2.0 ** -22 * gq.abs().clamp_min(1.0))
        z = torch.zeros(1, 128, C)
        return _tail_case(sd, f"t5_{s}_{q}", dtype, 1, 128, 1, 7, 51, extra=1.0, ref=lambda t, c: t["ff"][:, C * q:C * (q + 1)], o1=z, h=z, x=z, add=add.expand(128, C).reshape(1, 128, C))
    return make


def _t6(dtype):
    sd = neutral_sd(); g = _gen(16)
    sd[P + ".proj_out.weight"] = _r(g, C, C, 1, 1, sc=C ** -0.5); sd[P + ".proj_out.bias"] = _r(g, C, sc=0.1)
    return _tail_case(sd, "t6", dtype, 2, 128, 1, 77, 17, extra=1.0, ref=lambda t, c: t["out"], o1=torch.zeros(2, 128, C))


def _chain(B, f, HW, Lt, gate_shift=0.0, halves=1):
    def make(dtype):
        key = f"chain{gate_shift}"
        return _tail_case(rand_sd(0, gate_shift), key, dtype, B, HW, f, Lt, 1000 + 7 * B + Lt, extra="chain", ref=lambda t, c: t["out"], halves=halves)
    return make


def _coef(g, B, kind):
    a = 1 + 0.5 * _r(g, B, C); d = _r(g, B, C)
    if kind == "edge":                                                 # distinct per image, a = 0 for some channels, large d
        a[:, ::7] = 0.0
        d[:, 3::5] *= 100.0
    if kind == "one":
        a[:] = 1.0; d[:] = 0.0
    return torch.stack([a, d], -1).contiguous()


def _head_case(sd, sd_key, dtype, x, coef, groups, extra, ref, add=None):
    return dict(sd=sd, sd_key=sd_key, x=x.to(dtype), coef=coef, groups=groups, extra=extra, add=add, ref=ref)


def _head_all(t, c):
    return {"h": t["h"], "q": t["q"], "k": t["k"], "vt": t["v"].transpose(1, 2)}


def _h1(dtype):
    g = _gen(61)
    x = _r(g, 3, 128, C, sc=1.5).to(dtype); coef = _coef(g, 3, "edge")
    add = 2.0 ** -23 * ((x.double() * coef[:, None, :, 0].double()).abs() + coef[:, None, :, 1].double().abs())
    return _head_case(neutral_sd(), "h1", dtype, x, coef, {"h": ("h", None)}, 1.0, lambda t, c: {"h": t["xn"]}, add)


def _h2(dtype):
    sd = neutral_sd(); g = _gen(62)
    sd[P + ".proj_in.weight"] = _r(g, C, C, 1, 1, sc=C ** -0.5); sd[P + ".proj_in.bias"] = _r(g, C, sc=0.1)
    return _head_case(sd, "h2", dtype, _r(g, 3, 128, C), _coef(g, 3, "mild"), {"h": ("h", None)}, 1.0, _head_all)


def _h3(which):
    def make(dtype):
        sd = neutral_sd()
        gam, bet = ln_affine(which)
        sd[T + ".norm1.weight"] = gam.clone(); sd[T + ".norm1.bias"] = bet.clone()
        sd[T + ".attn1.to_q.weight"] = scaled_eye(); sd[T + ".attn1.to_k.weight"] = torch.eye(C); sd[T + ".attn1.to_v.weight"] = torch.eye(C)
        rows, cls = ln_rows(which, dtype)
        groups = {f"{o}.{c}": (o, s) for o in ("q", "k", "vt") for c, s in cls.items()}
        return _head_case(sd, "h3" + which, dtype, rows[None], _coef(_gen(63), 1, "one"), groups, 2.0, lambda t, c: {"q": t["n1"], "k": t["n1"], "vt": t["n1"].transpose(1, 2)})
    return make


def _h4(B, HW):
    def make(dtype):
        sd = rand_sd(3); g = _gen(64 + HW)
        return _head_case(sd, "h4", dtype, _r(g, B, HW, C, sc=1.5) + 0.3, _coef(g, B, "mild"), {o: (o, None) for o in ("h", "q", "k", "vt")}, "chain", _head_all)
    return make


T3_LT = [1, 7, 31, 32, 33, 64, 77, 95, 96]
CHAIN_SHAPES = [(1, 1, 128), (2, 1, 128), (3, 3, 128), (4, 2, 256), (6, 3, 128)]
CHAIN_LT = [1, 33, 77, 96]

CASES = ([Case("T1", "tail", _t1), Case("T2-A", "tail", _t2("A")), Case("T2-B", "tail", _t2("B")), Case("T2-C", "tail", _t2("C"))]
         + [Case(f"T3-{kind}-Lt{Lt}", "tail", _t3(Lt, kind)) for Lt in T3_LT for kind in ("ordinary", "onehot", "low")]
         + [Case("T4", "tail", _t4)]
         + [Case(f"T5-set{s}-q{q}", "tail", _t5(s, q)) for s in range(5) for q in range(4)]
         + [Case("T6", "tail", _t6)]
         + [Case(f"chain-B{B}f{f}HW{HW}-Lt{Lt}", "tail", _chain(B, f, HW, Lt)) for B, f, HW in CHAIN_SHAPES for Lt in CHAIN_LT]
         + [Case("chain-gate14-B2f1HW128-Lt77", "tail", _chain(2, 1, 128, 77, 14.0))]
         + [Case(f"chain-halves2-B{B}-Lt{Lt}", "tail", _chain(B, B, 128, Lt, halves=2)) for B in (1, 3) for Lt in (33, 77)]
         + [Case("H1", "head", _h1), Case("H2", "head", _h2), Case("H3-A", "head", _h3("A")), Case("H3-B", "head", _h3("B")), Case("H3-C", "head", _h3("C")),
            Case("H4-HW128", "head", _h4(3, 128)), Case("H4-HW256", "head", _h4(2, 256))])
BY_NAME = {c.name: c for c in CASES}

# E(dtype): the smallest `extra` at which the float32 oracle passes share() against the float64 mirror over every chain case (tail chains and
# H4), measured by tests/test_ttail_ref_cpu.py::test_chain_bar_is_twice_the_oracle_s_own_error; the bar is 2 E rounded up to an integer.
CHAIN_E = {torch.bfloat16: 7.9, torch.float16: 10.2}                # measured 7.87 (chain-halves2-B3-Lt33), 10.13 (chain-gate14-B2f1HW128-Lt77)
CHAIN_BAR = {torch.bfloat16: 16, torch.float16: 21}


def outputs(case_dict, kind, dtype, acc=torch.float32, mut=()):
    """{output name: tensor} of a made case as the kernel returns them (rounded): the oracle"""
    c = case_dict
    if kind == "tail":
        return {"out": tail(c["sd"], c["o1"], c["h"], c["x"], c["k"], c["vt"], c["f"], c["Lt"], dtype, acc=acc, mut=mut, halves=c["halves"])}
    return head(c["sd"], c["x"], c["coef"], dtype, acc=acc, mut=mut)


def reference(case_dict, kind, dtype):
    """{output name: float64 tensor}: the mirror's value of the stage under test BEFORE its own rounding (what _close's "one output rounding"
    is measured from), as the case's `ref` picks it from the taps; every earlier stage rounded as the kernel rounds it"""
    c, taps = case_dict, {}
    if kind == "tail":
        tail(c["sd"], c["o1"], c["h"], c["x"], c["k"], c["vt"], c["f"], c["Lt"], dtype, halves=c["halves"], taps=taps)
        B = c["o1"].shape[0] * c["halves"]
        return {"out": c["ref"](taps, c).reshape(B, -1, C)}
    head(c["sd"], c["x"], c["coef"], dtype, taps=taps)
    return c["ref"](taps, c)


def shares(case_dict, got, ref, dtype):
    """{group label: share of its bar} for the outputs `got` against `ref`"""
    c = case_dict
    extra = CHAIN_BAR[dtype] if c["extra"] == "chain" else c["extra"]
    out = {}
    for label, (name, rows) in c["groups"].items():
        g_, r_ = got[name], ref[name]
        a_ = c["add"]
        if rows is not None:
            if name == "vt":
                g_, r_ = g_[:, :, rows], r_[:, :, rows]
            else:
                g_, r_ = g_[:, rows], r_[:, rows]
                a_ = None if a_ is None else a_[:, rows]
        out[label] = share(g_, r_, dtype, extra, a_, slack=a_ is None)
    return out
