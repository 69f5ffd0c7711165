"""The compositing kernels alone on the crafted tile lists of tests/_composite_scene.py: every forward entry point with exact final_index, every
backward entry point per Gaussian against the float64 closed form (row metric and BARS of _composite_scene, formed on the CPU from the
reference's own float32-vs-float64 distance; tests/test_composite_vjp_cpu.py).

Inputs go through _redzone.on_device; outputs and workspaces start zero where the ABI requires it and NaN otherwise and must be finite afterwards;
the capacity padding of ids_sorted is 0.  Float atomics make no run-to-run promise of identical bits, so where two entry points compute the same
gradients (clamped with nothing above 1, abs against non-abs) each is held to the bars, not to the other's bits."""
import numpy as np
import pytest
import torch

import _composite_scene as cs
from _margins import within
from _redzone import on_device
from gaussctrl_amd import _lib as L
from gaussctrl_amd import gsplat_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = np.float64
PAD = 37
WIDTH = {"v_xy": 2, "v_conic": 3, "v_colors": 3, "v_opacity": 1, "v_extra": 1, "xy_abs": 2}


def _d(a):
    return on_device(torch.from_numpy(np.ascontiguousarray(a)), DEV)


def _h(t):
    return t.detach().cpu().numpy()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


class Inputs:
    """the device arrays of V views of one scene ([V][N][..], ids_sorted [V][M + pad] zero-padded); opac / background are view 0's when shared"""

    def __init__(self, name, V=1, shared=True, C=3, pad=0):
        self.scs = [cs.scene(name, v, not shared) for v in range(V)]
        s0 = self.scs[0]
        self.V, self.N, self.H, self.W, self.C, self.shared = V, s0["N"], s0["H"], s0["W"], C, shared
        self.tx, self.ty = s0["tiles"]
        self.M = len(s0["ids_sorted"])
        self.M_cap = self.M + pad
        cols = [cs.colors_nd(sc, C) for sc in self.scs]
        self.cols = cols
        ids = np.zeros((V, self.M_cap), np.int32)
        for v, sc in enumerate(self.scs):
            ids[v, :self.M] = sc["ids_sorted"]
        self.ids, self.bins = _d(ids), _d(np.stack([sc["tile_bins"] for sc in self.scs]))
        self.xys, self.conics = _d(np.stack([sc["xys"] for sc in self.scs])), _d(np.stack([sc["conics"] for sc in self.scs]))
        self.colors, self.extra = _d(np.stack([c for c, _ in cols])), _d(np.stack([sc["extra"] for sc in self.scs]))
        self.opac = _d(s0["opac"] if shared else np.stack([sc["opac"] for sc in self.scs]))
        self.bg = _d(cols[0][1] if shared else np.stack([b for _, b in cols]))

    def head(self):
        return (L.i32(self.V), L.i64(self.N), L.i64(self.M_cap), L.i32(int(self.shared)), L.i32(int(self.shared)))

    def size(self):
        return (L.i32(self.H), L.i32(self.W), L.i32(self.tx), L.i32(self.ty))

    def splats(self):
        return (L.ptr(self.ids), L.ptr(self.bins), L.ptr(self.xys), L.ptr(self.conics), L.ptr(self.colors), L.ptr(self.opac))

    def ref_forward(self, v):
        return cs.forward(self.scs[v], F64, *self.cols[v])


def _forward(inp, entry):
    """-> dict(image [V,H,W,C], extra [V,H,W] | None, final_Ts, final_index) of one forward entry point, outputs NaN- / -7-filled before"""
    V, H, W, C = inp.V, inp.H, inp.W, inp.C
    img, fT = _nan(V, H, W, C), _nan(V, H, W)
    fi = torch.full((V, H, W), -7, dtype=torch.int32, device=DEV)
    E = _nan(V, H, W) if entry in ("fwd_extra", "views") else None
    lib, st = L.lib(), L.stream_ptr()
    if entry in ("fwd", "fwd_extra"):
        L.check(lib.gc_rasterize_fwd(*inp.size(), *inp.splats(), L.ptr(inp.extra if E is not None else None), L.ptr(inp.bg), L.ptr(img), L.ptr(E),
                                     L.ptr(fT), L.ptr(fi), st), "gc_rasterize_fwd")
    elif entry == "views":
        L.check(lib.gc_rasterize_fwd_views(*inp.head(), *inp.size(), *inp.splats(), L.ptr(inp.extra), L.ptr(inp.bg), L.ptr(img), L.ptr(E), L.ptr(fT),
                                           L.ptr(fi), st), "gc_rasterize_fwd_views")
    else:
        L.check(lib.gc_rasterize_nd_fwd(*inp.size(), L.i32(C), *inp.splats(), L.ptr(inp.bg), L.ptr(img), L.ptr(fT), L.ptr(fi), st), "gc_rasterize_nd_fwd")
    torch.cuda.synchronize()
    return dict(image=img, extra=E, final_Ts=fT, final_index=fi)


def _check_forward(label, inp, fw):
    for v in range(inp.V):
        ref = inp.ref_forward(v)
        assert np.array_equal(_h(fw["final_index"][v]), ref["final_index"]), f"{label}: final_index differs from the float64 reference"
        got = {k: (None if fw[k] is None else _h(fw[k][v])) for k in ("image", "extra", "final_Ts")}
        for k, e in cs.forward_errors(got, ref).items():
            within(f"{label} view {v}: forward {k}", e, cs.FWD_BARS[k])


def _backward(entry, inp, fw, cots, clamp=False, init=None):
    """one backward entry point through the raw ABI.  cots: per view {"v_out", "v_alpha" | None, "v_depth" | None}; init: {key: [V,N,w] array}
    the outputs start from (default zeros).  -> {key: tensor [V, N, w]}"""
    V, N, C = inp.V, inp.N, inp.C
    depth = entry == "depth" or (entry == "abs" and cots[0]["v_depth"] is not None)
    keys = ["v_xy", "v_conic", "v_colors", "v_opacity"] + (["v_extra"] if depth else []) + (["xy_abs"] if entry == "abs" else [])
    out = {}
    for k in keys:
        w = C if k == "v_colors" else WIDTH[k]
        out[k] = torch.zeros(V, N, w, dtype=torch.float32, device=DEV) if init is None else _d(init[k].astype(np.float32))
    v_out = _d(np.stack([c["v_out"] for c in cots]))
    v_al = None if cots[0]["v_alpha"] is None else _d(np.stack([c["v_alpha"] for c in cots]))
    pre = fw["image"] if clamp else None
    quartet = [None] * 4
    if depth:
        zero = np.zeros((inp.H, inp.W), np.float32)
        v_dp = _d(np.stack([zero if c["v_depth"] is None else c["v_depth"] for c in cots]))
        dep = _d(np.stack([cs.finalize_depth(_h(fw["extra"][v]), _h(fw["final_Ts"][v])) for v in range(V)]))
        quartet = [inp.extra, dep, v_dp, out["v_extra"]]
    lib, st = L.lib(), L.stream_ptr()
    sav = (L.ptr(inp.bg), L.ptr(fw["final_Ts"]), L.ptr(fw["final_index"]), L.ptr(v_out), L.ptr(v_al))
    grads = tuple(L.ptr(out[k]) for k in ("v_xy", "v_conic", "v_colors", "v_opacity"))
    if entry == "bwd":
        L.check(lib.gc_rasterize_bwd(*inp.size(), L.i64(N), *inp.splats(), *sav, *grads, st), entry)
    elif entry == "clamped":
        L.check(lib.gc_rasterize_bwd_clamped(*inp.size(), L.i64(N), *inp.splats(), *sav, L.ptr(fw["image"]), *grads, st), entry)
    elif entry == "views":
        L.check(lib.gc_rasterize_bwd_views(*inp.head(), *inp.size(), *inp.splats(), *sav, L.ptr(pre), *grads, st), entry)
    elif entry == "depth":
        L.check(lib.gc_rasterize_bwd_depth_views(*inp.head(), *inp.size(), *inp.splats(), *sav, L.ptr(pre), *grads, *(L.ptr(q) for q in quartet), st), entry)
    elif entry == "abs":
        L.check(lib.gc_rasterize_bwd_abs_views(*inp.head(), *inp.size(), *inp.splats(), *sav, L.ptr(pre), *grads, *(L.ptr(q) for q in quartet),
                                               L.ptr(out["xy_abs"]), st), entry)
    else:
        L.check(lib.gc_rasterize_nd_bwd(*inp.size(), L.i64(N), L.i32(C), *inp.splats(), *sav, *grads, st), entry)
    torch.cuda.synchronize()
    return out


def _check_rows(label, got, ref, before=None, faint=None):
    """one view's outputs {key: array [N, w]} against pair_backward's result by the row metric at BARS; before: what the buffers held"""
    for k, g in got.items():
        g = np.asarray(g, F64)
        assert np.isfinite(g).all(), (label, k)
        want, A = (ref["xy_abs"], ref["v_xy"][1]) if k == "xy_abs" else ref[k]
        slack = None
        if before is not None:
            x = np.asarray(before[k], F64)
            g, slack = g - x, 2.0 ** -23 * np.linalg.norm(x.reshape(x.shape[0], -1), axis=1)
        worst, n = cs.row_errors(g.reshape(want.shape), want, A, slack)
        within(f"{label}: {k} worst row error ({n} rows)", worst, cs.BARS[k])
        if faint is not None and k in faint and faint[k].any():
            within(f"{label}: {k} worst FAINT row error ({int(faint[k].sum())} rows)", cs.row_errors(g.reshape(want.shape), want, A, slack, faint[k])[0],
                   cs.BARS[k])


def _prepare(name, V=1, shared=True, C=3, pad=0):
    inp = Inputs(name, V, shared, C, pad)
    fw = _forward(inp, "views" if C == 3 else "nd")
    _check_forward(f"{name} V={V}", inp, fw)
    return inp, fw


def _faint(inp, v, ref):
    """the faint rows of `opaque`, reported on their own so that the margins log shows what they use"""
    return cs.faint_rows(inp.scs[v], ref) if inp.scs[v]["name"] == "opaque" else None


def _refs(inp, cset, depth=False, clamp=False):
    return [cs.reference(sc, cset, depth, inp.C, clamp) for sc in inp.scs]


def _cots(inp, cset, depth=False):
    return [cs.cotangents(sc, cset, inp.C, depth) for sc in inp.scs]


# ---------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", cs.SCENES)
def test_forward(name):
    one = Inputs(name)
    base = None
    for entry in ("fwd", "fwd_extra", "views"):
        fw = _forward(one, entry)
        _check_forward(f"{name} {entry}", one, fw)
        if base is None:
            base = fw
        for k in ("final_Ts", "final_index"):
            assert torch.equal(fw[k], base[k]), (entry, k)          # fwd_step is one piece of code for all of them: the same bits
    three = Inputs(name, 3, False, 3, PAD)
    _check_forward(f"{name} views x3", three, _forward(three, "views"))
    for C in (1, 4, 33):
        nd = Inputs(name, C=C)
        fw = _forward(nd, "nd")
        _check_forward(f"{name} nd C={C}", nd, fw)
        assert torch.equal(fw["final_Ts"], base["final_Ts"]) and torch.equal(fw["final_index"], base["final_index"])


# ---------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("cset", "abc")
@pytest.mark.parametrize("name", cs.SCENES)
def test_bwd(name, cset):
    """gc_rasterize_bwd through ops._rasterize_bwd"""
    inp, fw = _prepare(name)
    cot = _cots(inp, cset)[0]
    got = ops._rasterize_bwd(inp.H, inp.W, (inp.tx, inp.ty, 1), inp.N, inp.ids[0], inp.bins[0], inp.xys[0], inp.conics[0], inp.colors[0], inp.opac,
                             inp.bg, fw["final_Ts"][0], fw["final_index"][0], _d(cot["v_out"]), None if cot["v_alpha"] is None else _d(cot["v_alpha"]))
    torch.cuda.synchronize()
    ref = _refs(inp, cset)[0]
    _check_rows(f"{name} {cset} bwd", dict(zip(cs.KEYS, (_h(g) for g in got))), ref, faint=_faint(inp, 0, ref))


@pytest.mark.parametrize("name,cset", [("opaque", "a"), ("opaque", "b"), ("deep", "a"), ("tiny", "a")])
def test_bwd_clamped(name, cset):
    """gc_rasterize_bwd_clamped: v_out masked where the pre-clamp image exceeds 1 (opaque); nothing exceeds 1 in deep and tiny"""
    inp, fw = _prepare(name)
    pre = _h(fw["image"][0])
    assert np.array_equal(pre > 1, inp.ref_forward(0)["image"] > 1)
    assert bool((pre > 1).any()) == (name == "opaque")
    got = _backward("clamped", inp, fw, _cots(inp, cset), clamp=True)
    ref = _refs(inp, cset, clamp=True)[0]
    _check_rows(f"{name} {cset} clamped", {k: _h(g[0]) for k, g in got.items()}, ref, faint=_faint(inp, 0, ref))


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("name", cs.SCENES)
def test_bwd_views(name, shared):
    """gc_rasterize_bwd_views, three views of different geometry and cotangents (and, unshared, opacities and backgrounds), M_cap = M + 37"""
    inp, fw = _prepare(name, 3, shared, 3, PAD)
    for cset in "ab":                                   # a: v_out_alpha set, b: NULL
        for clamp in (False, True):
            got = _backward("views", inp, fw, _cots(inp, cset), clamp=clamp)
            for v, ref in enumerate(_refs(inp, cset, clamp=clamp)):
                _check_rows(f"{name} shared={shared} {cset} clamp={clamp} view {v}", {k: _h(g[v]) for k, g in got.items()}, ref, faint=_faint(inp, v, ref))


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("name", cs.SCENES)
def test_bwd_depth_views(name, V):
    inp, fw = _prepare(name, V, V == 1, 3, PAD if V > 1 else 0)
    if name == "opaque":
        assert (_h(fw["final_Ts"]) == 1).any()                        # pixels of alpha 0: no depth gradient
    for cset in "ad":
        got = _backward("depth", inp, fw, _cots(inp, cset, True))
        for v, ref in enumerate(_refs(inp, cset, True)):
            _check_rows(f"{name} V={V} {cset} depth view {v}", {k: _h(g[v]) for k, g in got.items()}, ref, faint=_faint(inp, v, ref))


@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("name", cs.SCENES)
def test_bwd_abs_views(name, depth):
    """v_xy_abs against xy_abs at the v_xy bar; the signed outputs at their own bars"""
    inp, fw = _prepare(name, 3, False, 3, PAD)
    got = _backward("abs", inp, fw, _cots(inp, "a", depth))
    assert ("v_extra" in got) == depth
    for v, ref in enumerate(_refs(inp, "a", depth)):
        _check_rows(f"{name} abs depth={depth} view {v}", {k: _h(g[v]) for k, g in got.items()}, ref)


@pytest.mark.parametrize("C", [1, 4, 33])
@pytest.mark.parametrize("name", ["deep", "opaque"])
def test_nd_bwd(name, C):
    inp, fw = _prepare(name, C=C)
    for cset in "ab":
        got = _backward("nd", inp, fw, _cots(inp, cset))
        _check_rows(f"{name} nd C={C} {cset}", {k: _h(g[0]) for k, g in got.items()}, _refs(inp, cset)[0])


@pytest.mark.parametrize("entry", ["bwd", "clamped", "views", "depth", "abs", "nd"])
def test_accumulates_onto_its_outputs(entry):
    """every backward adds into its outputs: from a seeded non-zero x, (result - x) is held to the bar plus 2^-23 |x_row|.  x is 0.1 of the row's
    term-wise sum A times a normal draw (a row no term reaches gets a plain normal draw, and must come back bit for bit)"""
    C = 4 if entry == "nd" else 3
    V = 1 if entry in ("bwd", "clamped", "nd") else 3
    inp, fw = _prepare("stop", V, V == 1, C, PAD if V > 1 else 0)
    depth = entry in ("depth", "abs")
    refs = _refs(inp, "a", depth, entry == "clamped")
    g = np.random.default_rng(4242)
    init = {}
    for k in ["v_xy", "v_conic", "v_colors", "v_opacity"] + (["v_extra"] if depth else []) + (["xy_abs"] if entry == "abs" else []):
        A = np.stack([r["v_xy"][1] if k == "xy_abs" else r[k][1] for r in refs])
        an = np.linalg.norm(A, axis=2, keepdims=True)
        init[k] = (g.normal(size=A.shape) * np.where(an > 0, 0.1 * an, 1.0)).astype(np.float32)
    got = _backward(entry, inp, fw, _cots(inp, "a", depth), clamp=entry == "clamped", init=init)
    for v, ref in enumerate(refs):
        _check_rows(f"stop {entry} accumulate view {v}", {k: _h(t[v]) for k, t in got.items()}, ref, before={k: x[v] for k, x in init.items()})
