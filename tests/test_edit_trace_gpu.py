"""GPU tests of edit-region tracing (include/gaussctrl_trace.h; csrc/raster_trace.hip, k_adam_rows of csrc/train_step.hip;
gsplat_ops.trace_masks_views, gaussctrl_amd/edit_region.py, train_ops.FusedAdam.row_select, GaussCtrlPipelineConfig.edit_region).

The traced sums are checked against the fp64 oracle (oracle/raster_torch.py::rasterize with two unit colour channels, fed the device's own
projected geometry and tile lists of the view: d/d colors of sum(out[..., 0] * mask + out[..., 1]) is (w_in, w_all)) at the project's
leaf-gradient bar, 1e-3 of the array's maximum (float atomics).  Oracle sums are computed once per (scene, mode, view)
and kept as numpy arrays for every test of the module, the guarded re-runs included (the device's projection and binning are
deterministic, so the lists they were computed on are the lists of every later call).

Every input is made with a torch factory and an explicit device, so that the red-zone re-runs at the end of the file (tests/_redzone.py)
carve them from the arena."""
import math
import types

import numpy as np
import pytest
import torch

from _margins import within
from _redzone import guard
from gaussctrl_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (0.1, 0.2, 0.3)

# (name, N, W, H, fx, scale_mean)
TINY = ("tiny", 7, 33, 17, 40.0, 0.3)                 # part-filled tiles, 4 of the 7 Gaussians visible
SMALL0 = ("small0", 5000, 200, 136, 180.0, 0.03)      # test_raster_nd_gpu.SMALL[0]: 13 x 9 tiles, lists of up to ~340 entries
DENSE = ("dense", 4000, 48, 40, 40.0, 0.08)           # 3 x 3 tiles with lists of ~2000 entries: many LDS batches, pixels that saturate
# the selection scene: 2000 Gaussians of ONE size (0.02) and ONE opacity (sigmoid(-1)) at 200 x 136.  The rows the comparison has to leave
# out are those within 2e-3 max(w_all) of the threshold; in the module's other scenes a few large splats own max(w_all) and 74 - 81 % of the
# visible rows would be left out (fp64 oracle on the CPU, its own fp32 projection); here it is 1.0 % of 1514 visible rows, 758 selected.
SELECT = ("select", 2000, 200, 136, 180.0, 0.02)


def _t(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def _params(scene):
    name, N, W, H, fx, sm = scene
    P = syn.make_gaussians(N, seed=3, scale_mean=sm)
    if name == "select":
        P["scales"][:] = math.log(sm)
        P["opacities"][:] = -1.0
    return {k: _t(v) for k, v in P.items()}


def _cams(scene, C):
    from gaussctrl_amd.camera import camera_to_gsplat
    _, _, W, H, fx, _ = scene
    return [camera_to_gsplat(c2w, fx, fx * 0.99, W / 2 + 1.3, H / 2 - 2.1, W, H) for c2w in syn.make_cameras(C, seed=4)]


def _leaves(tp):
    return [tp[k] for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest")]


def _masks(kinds, H, W):
    """[len(kinds), H, W] float32: 'half' = the left half plane, 'ramp' = a soft ramp over the width (non-binary), 'ones', 'zeros'"""
    out = torch.zeros(len(kinds), H, W, dtype=torch.float32, device=DEV)
    for k, kind in enumerate(kinds):
        if kind == "half":
            out[k, :, :W // 2] = 1.0
        elif kind == "ramp":
            out[k] = torch.linspace(0.0, 1.0, W, device=DEV)[None, :].expand(H, W)
        elif kind == "ones":
            out[k] = 1.0
        else:
            assert kind == "zeros"
    return out


def _aux(aa):
    from gaussctrl_amd import gsplat_ops as ops
    aux = ops.RenderAux()
    aux.antialiased = aa
    return aux


def _trace(tp, cams, masks, aa=False):
    from gaussctrl_amd import gsplat_ops as ops
    N = tp["means"].shape[0]
    w_in = torch.zeros(N, dtype=torch.float32, device=DEV)
    w_all = torch.zeros(N, dtype=torch.float32, device=DEV)
    ops.trace_masks_views(*_leaves(tp), cams, masks, w_in, w_all, _aux(aa))
    return w_in, w_all


def _tile_saturates(xys, conics, opac, ids, s, e, tx, ty, H, W):
    """does some pixel of tile (tx, ty) reach the T stop within its list [s, e)?  The oracle's expressions, in float64"""
    gid = ids[s:e].long()
    py, px = torch.meshgrid(torch.arange(ty * 16, min(ty * 16 + 16, H), dtype=torch.float64, device=DEV),
                            torch.arange(tx * 16, min(tx * 16 + 16, W), dtype=torch.float64, device=DEV), indexing="ij")
    dx = xys[gid, 0].double()[None, :] - px.reshape(-1, 1)
    dy = xys[gid, 1].double()[None, :] - py.reshape(-1, 1)
    cn = conics[gid].double()
    sigma = 0.5 * (cn[:, 0] * dx * dx + cn[:, 2] * dy * dy) + cn[:, 1] * dx * dy
    alpha = torch.clamp(opac[gid].double()[None, :] * torch.exp(-sigma), max=0.999)
    valid = (sigma >= 0) & (alpha >= 1.0 / 255.0)
    T_incl = torch.cumprod(torch.where(valid, 1 - alpha, torch.ones_like(alpha)), dim=1)
    return bool((valid & (T_incl <= 1e-4)).any())


_ORACLE = {}


def _oracle_views(scene, tp, cams, kinds, aa):
    """per view c: (w_in, w_all) of the fp64 oracle under mask kinds[c] as float64 numpy arrays, on the device's own geometry and lists of
    the view; plus what the fixture is: the longest tile list and whether a pixel of that tile reaches the T stop"""
    key = (scene[0], aa, tuple(kinds))
    if key not in _ORACLE:
        from gaussctrl_amd import gsplat_ops as ops
        from oracle import raster_torch as rt
        _, N, W, H, _, _ = scene
        with torch.no_grad():
            fr = ops._views_front(*_leaves(tp), cams, 0, _aux(aa))
        masks = _masks(kinds, H, W)
        cnt = fr.cnt.cpu()
        views, longest, saturates = [], 0, False
        for c in range(len(cams)):
            xys, conics = fr.xys[c], fr.conics[c]
            opac = fr.opac if fr.shared_op else fr.opac[c]
            ids, bins = fr.ids_s[c, :int(cnt[c])], fr.bins[c].cpu()
            col = torch.ones(N, 2, dtype=torch.float64, device=DEV, requires_grad=True)
            with torch.device(DEV):
                out, _, _, _ = rt.rasterize(xys.double(), conics.double(), col, opac.double(), ids, bins, H, W, fr.tb,
                                            torch.zeros(2, dtype=torch.float64, device=DEV))
            (out[..., 0] * masks[c].double() + out[..., 1]).sum().backward()
            views.append((col.grad[:, 0].cpu().numpy(), col.grad[:, 1].cpu().numpy()))
            lens = (bins[:, 1] - bins[:, 0])
            t = int(lens.argmax())
            if int(lens[t]) > longest:
                longest = int(lens[t])
                saturates = _tile_saturates(xys, conics, opac, ids, int(bins[t, 0]), int(bins[t, 1]), t % fr.tb[0], t // fr.tb[0], H, W)
        _ORACLE[key] = (views, longest, saturates)
    return _ORACLE[key]


def _sum_close(what, got, ref):
    """the leaf-gradient bar: |got - ref| <= 1e-3 of max |ref| on every Gaussian"""
    ref = np.asarray(ref, np.float64)
    d = np.abs(got.double().cpu().numpy() - ref).max() if ref.size else 0.0
    within(f"{what}: max |trace - oracle| / max", d, 1e-3 * np.abs(ref).max())


KINDS = ("half", "ramp", "ones")          # a different mask per view


# ------------------------------------------------------------------------------------------------------------------ 1. sums vs the oracle
@pytest.mark.parametrize("scene,aa", [(TINY, False), (SMALL0, False), (DENSE, False), (SMALL0, True)], ids=["tiny", "small0", "dense", "small0-aa"])
def test_sums_vs_fp64_oracle(scene, aa):
    """C = 1 per view (half plane, soft ramp, all ones) against the oracle; C = 3 in one launch against the sum of the three single-view
    calls (1e-5 of the max: the same additions in another order) and against the oracle; all ones: w_in = w_all and sum(w_all) =
    sum(1 - T_final) of render_views on the same cameras; all zeros: w_in stays exactly 0; the selection made from the sums is the rule
    evaluated on them."""
    from gaussctrl_amd import edit_region as er, gsplat_ops as ops
    name, N, W, H, _, _ = scene
    tp, cams = _params(scene), _cams(scene, 3)
    views, longest, saturates = _oracle_views(scene, tp, cams, KINDS, aa)
    if name == "dense":                    # the fixture itself: a second LDS batch and the T stop are on this scene's path
        assert longest > 256 and saturates, (longest, saturates)
    masks = _masks(KINDS, H, W)
    single = []
    for c in range(3):
        w_in, w_all = _trace(tp, cams[c:c + 1], masks[c:c + 1], aa)
        _sum_close(f"{name} view {c} ({KINDS[c]}) w_in", w_in, views[c][0])
        _sum_close(f"{name} view {c} ({KINDS[c]}) w_all", w_all, views[c][1])
        single.append((w_in, w_all))
    # all ones (view 2)
    w_in, w_all = single[2]
    within(f"{name} ones: max |w_in - w_all| / max", float((w_in - w_all).abs().max()), 1e-5 * float(w_all.abs().max()))
    # C = 3
    w_in3, w_all3 = _trace(tp, cams, masks, aa)
    s_in, s_all = single[0][0] + single[1][0] + single[2][0], single[0][1] + single[1][1] + single[2][1]
    within(f"{name} C=3: max |w_in - sum of single views| / max", float((w_in3 - s_in).abs().max()), 1e-5 * float(s_in.abs().max()))
    within(f"{name} C=3: max |w_all - sum of single views| / max", float((w_all3 - s_all).abs().max()), 1e-5 * float(s_all.abs().max()))
    _sum_close(f"{name} C=3 w_in", w_in3, sum(v[0] for v in views))
    _sum_close(f"{name} C=3 w_all", w_all3, sum(v[1] for v in views))
    with torch.no_grad():
        _, alpha, _ = ops.render_views(*_leaves(tp), cams, torch.tensor(BG, dtype=torch.float32, device=DEV), False, 0, _aux(aa))
    a = float(alpha.double().sum())
    within(f"{name}: |sum w_all - sum (1 - T_final)| / sum", abs(float(w_all3.double().sum()) - a), 1e-4 * a)
    # all zeros: nothing but zeros is ever added to w_in
    z_in, z_all = _trace(tp, cams, _masks(("zeros",) * 3, H, W), aa)
    assert int(torch.count_nonzero(z_in)) == 0
    within(f"{name} zeros: max |w_all - w_all of the masked call| / max", float((z_all - w_all3).abs().max()), 1e-5 * float(w_all3.abs().max()))
    # the selection from these sums: exactly the rule in float32, count = the number selected, never-seen rows unselected
    for thr, mw in ((0.5, 0.0), (0.25, float(w_all3.median())), (-1.0, -1.0)):
        sel, n = er.select(w_in3, w_all3, thr, mw)
        want = (w_all3 != 0) & (w_all3 > mw) & (w_in3 > thr * w_all3)
        assert sel.dtype == torch.uint8 and torch.equal(sel.bool(), want) and n == int(sel.sum()) == int(want.sum())
        assert int(sel[w_all3 == 0].sum()) == 0 and int(sel[w_all3 <= mw].sum()) == 0


def test_empty_and_all_culled():
    from gaussctrl_amd import _lib as L, edit_region as er
    from gaussctrl_amd.camera import camera_to_gsplat
    # N = 0: through the host layer (nothing to add) and through the C ABI (no per-Gaussian array has an address)
    P = syn.make_gaussians(0, seed=1)
    tp = {k: _t(v) for k, v in P.items()}
    c2w = syn.look_at_c2w(np.array([0.0, -2.0, 0.0]), np.zeros(3))
    cams = [camera_to_gsplat(c2w, 100.0, 100.0, 32.0, 32.0, 64, 64)] * 2
    w_in, w_all = _trace(tp, cams, _masks(("ones", "half"), 64, 64))
    assert w_in.shape == (0,) and w_all.shape == (0,)
    null = L.ptr(None)
    assert L.lib().gc_trace_mask_views(L.i32(2), L.i64(0), L.i64(0), L.i32(1), L.i32(64), L.i32(64), L.i32(4), L.i32(4), null, null, null, null, null,
                                       null, null, null, L.stream_ptr()) == 0
    sel, n = er.select(w_in, w_all, 0.5, 0.0)
    assert sel.shape == (0,) and n == 0
    # every Gaussian behind the camera: no list entry, nothing is added, nothing is selected
    P = syn.make_gaussians(500, seed=1)
    P["means"][:] = [0, -5, 0]
    tp = {k: _t(v) for k, v in P.items()}
    w_in, w_all = _trace(tp, cams, _masks(("ones", "half"), 64, 64))
    assert int(torch.count_nonzero(w_in)) == 0 and int(torch.count_nonzero(w_all)) == 0
    sel, n = er.select(w_in, w_all, -1.0, -1.0)
    assert n == 0 and int(sel.sum()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 2. the composed form
def test_trace_matches_the_composed_form():
    """what a caller could write with the existing operators: a 2-channel rasterize_gaussians forward + backward with colors = 1 and
    v_out = (mask, 1) returns the same sums in v_colors -- on SMALL0 with the gsplat-box lists of the operator surface"""
    from gaussctrl_amd import _lib as L, gsplat_ops as ops
    from test_raster_nd_gpu import _lists, _projected
    _, N, W, H, fx, sm = SMALL0
    xys, depths, radii, conics, nth, opac = _projected(N, W, H, fx, sm)
    tb, ids, bins = _lists(xys, depths, radii, nth, W, H)
    mask = _masks(("ramp",), H, W)[0] * _masks(("half",), H, W)[0] + 0.25            # non-binary, non-zero everywhere
    colors = torch.ones(N, 2, dtype=torch.float32, device=DEV, requires_grad=True)
    out = ops.rasterize_gaussians(xys, depths, radii, conics, nth, colors, opac, H, W, background=torch.zeros(2, dtype=torch.float32, device=DEV))
    (out[..., 0] * mask + out[..., 1]).sum().backward()
    w_in = torch.zeros(N, dtype=torch.float32, device=DEV)
    w_all = torch.zeros(N, dtype=torch.float32, device=DEV)
    op = opac.reshape(-1).contiguous()
    L.check(L.lib().gc_trace_mask_views(L.i32(1), L.i64(N), L.i64(ids.numel()), L.i32(1), L.i32(H), L.i32(W), L.i32(tb[0]), L.i32(tb[1]), L.ptr(ids),
                                        L.ptr(bins), L.ptr(xys), L.ptr(conics), L.ptr(op), L.ptr(mask.contiguous()), L.ptr(w_in), L.ptr(w_all),
                                        L.stream_ptr()), "gc_trace_mask_views")
    assert float(colors.grad[:, 1].max()) > 0
    _sum_close("composed form w_in", w_in, colors.grad[:, 0].double().cpu().numpy())
    _sum_close("composed form w_all", w_all, colors.grad[:, 1].double().cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 3. selection
def test_selection_vs_the_rule_on_the_oracle_sums():
    """gc_trace_select on the device's sums against the rule on the oracle's, on the rows that are decided: |w_in - thr w_all| > 2e-3
    max(w_all), twice the sum bar since both sums may be off by it.  At most 5 % of the visible rows may be left out (SELECT above: 1.0 %
    with the oracle alone)."""
    from gaussctrl_amd import edit_region as er
    _, N, W, H, _, _ = SELECT
    thr = 0.5
    tp, cams = _params(SELECT), _cams(SELECT, 1)
    (o_in, o_all), = _oracle_views(SELECT, tp, cams, ("half",), False)[0]
    w_in, w_all = _trace(tp, cams, _masks(("half",), H, W))
    _sum_close("select scene w_in", w_in, o_in)
    _sum_close("select scene w_all", w_all, o_all)
    sel, n = er.select(w_in, w_all, thr, 0.0)
    sel = sel.cpu().numpy().astype(bool)
    assert n == int(sel.sum())
    visible = o_all > 0
    decided = np.abs(o_in - thr * o_all) > 2e-3 * o_all.max()
    within("selection: share of the visible rows left out", float((visible & ~decided).sum()) / float(visible.sum()), 0.05)
    want = visible & (o_in > thr * o_all)
    assert int(visible.sum()) > 1000 and 0.25 * visible.sum() < want.sum() < 0.75 * visible.sum()
    assert np.array_equal(sel[decided], want[decided]), int((sel[decided] != want[decided]).sum())
    assert not sel[~visible].any()
    # min_weight: rows at or below it are unselected, the others keep their decision
    mw = float(np.median(o_all[visible]))
    sel2, n2 = er.select(w_in, w_all, thr, mw)
    sel2 = sel2.cpu().numpy().astype(bool)
    wa = w_all.cpu().numpy()
    assert n2 == int(sel2.sum()) and 0 < n2 < n
    assert not sel2[wa <= mw].any() and np.array_equal(sel2[wa > mw], sel[wa > mw])


# ------------------------------------------------------------------------------------------------------------------ 4. row-masked Adam
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("rows", [1, 5, 1027])
@pytest.mark.parametrize("rf", [1, 3, 4, 45])
def test_adam_step_rows(rows, rf):
    """two consecutive steps per select pattern: selected rows get the bits of gc_adam_step on a copy, every other row of the parameter and
    of both moments keeps its bits.  rf = 3 and 45 put 16-byte chunks across rows; rows x rf = 5, 15, 1027, 3081 leave a scalar tail."""
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    g = torch.Generator(device=DEV).manual_seed(rows * 100 + rf)
    n = rows * rf

    def carved(values, dtype=torch.float32):                  # a buffer of its own from a factory (the red-zone re-run carves it), then filled
        out = torch.empty(values.shape, dtype=dtype, device=DEV)
        out.copy_(values)
        return out

    patterns = {"none": torch.zeros(rows, dtype=torch.uint8, device=DEV), "all": torch.full((rows,), 7, dtype=torch.uint8, device=DEV),   # any non-zero byte selects
                "alternating": carved(torch.arange(rows, device=DEV) % 2, torch.uint8),
                "random 10 %": carved(torch.rand(rows, device=DEV, generator=g) < 0.1, torch.uint8)}
    hyper = (L.f32(1.6e-4), L.f32(0.9), L.f32(0.999), L.f32(1e-15))
    for name, sel in patterns.items():
        p = torch.randn(rows, rf, device=DEV, generator=g)
        m = carved(torch.randn(rows, rf, device=DEV, generator=g) * 1e-3)
        v = carved(torch.rand(rows, rf, device=DEV, generator=g) * 1e-6)
        on = sel.bool()
        for step in (1, 2):
            grad = carved(torch.randn(rows, rf, device=DEV, generator=g) * 1e-2)
            before = [t.clone() for t in (p, m, v)]
            ref = [t.clone() for t in (p, m, v)]
            L.check(lib.gc_adam_step(L.ptr(ref[0]), L.ptr(grad), L.ptr(ref[1]), L.ptr(ref[2]), L.i64(n), *hyper, L.i32(step), L.stream_ptr()), "gc_adam_step")
            L.check(lib.gc_adam_step_rows(L.ptr(p), L.ptr(grad), L.ptr(m), L.ptr(v), L.i64(rows), L.i32(rf), L.ptr(sel), *hyper, L.i32(step),
                                          L.stream_ptr()), "gc_adam_step_rows")
            for what, got, r, b in zip(("param", "exp_avg", "exp_avg_sq"), (p, m, v), ref, before):
                assert torch.equal(_bits(got[on]), _bits(r[on])), (name, step, what, "selected rows")
                assert torch.equal(_bits(got[~on]), _bits(b[~on])), (name, step, what, "unselected rows")
            if on.any():
                assert not torch.equal(p[on], before[0][on])


def test_fused_adam_row_select():
    """FusedAdam.row_select: None is gc_adam_step; set, a parameter with that many rows steps in the selected rows only and a parameter of
    another row count steps whole"""
    from gaussctrl_amd.train_ops import FusedAdam
    g = torch.Generator(device=DEV).manual_seed(5)
    a0, b0 = torch.randn(9, 15, 3, device=DEV, generator=g), torch.randn(4, 3, device=DEV, generator=g)
    ga, gb = torch.randn(9, 15, 3, device=DEV, generator=g), torch.randn(4, 3, device=DEV, generator=g)
    sel = torch.tensor([1, 0, 0, 1, 0, 1, 1, 0, 0], dtype=torch.uint8, device=DEV)

    def run(row_select):
        a, b = torch.nn.Parameter(a0.clone()), torch.nn.Parameter(b0.clone())
        opt = FusedAdam([a, b], lr=1e-2)
        assert opt.row_select is None
        opt.row_select = row_select
        for _ in range(2):
            a.grad, b.grad = ga.clone(), gb.clone()
            opt.step()
        return a.detach(), b.detach(), opt.state[a]

    fa, fb, _ = run(None)
    ra, rb, st = run(sel)
    on = sel.bool()
    assert torch.equal(_bits(ra[on]), _bits(fa[on])) and torch.equal(_bits(ra[~on]), _bits(a0[~on])) and torch.equal(_bits(rb), _bits(fb))
    assert int(torch.count_nonzero(st["exp_avg"][~on])) == 0 and int(torch.count_nonzero(st["exp_avg_sq"][~on])) == 0
    assert not torch.equal(ra[on], a0[on])


# ------------------------------------------------------------------------------------------------------------------ 5. end to end
def _edit_run(P, cams, edit_region):
    """render_reverse (masks stored, traced when asked) and 5 training iterations of the stand-alone model with its callbacks: the cull of
    step 30000 falls after the first.  The diffusion side of render_reverse (VAE encode, DDIM inversion, text encoder) is stubbed: nothing of
    it reaches the trace or the training.  Returns (model, initial row of every surviving row, the selection before training)."""
    from gaussctrl_amd.gc_config import build_optimizers
    from gaussctrl_amd.gc_model import GaussCtrlModel, GaussCtrlModelConfig
    from gaussctrl_amd.gc_pipeline import GaussCtrlPipeline, GaussCtrlPipelineConfig, SimpleDataManager
    from gaussctrl_amd.gc_trainer import TrainingCallbackAttributes
    model = GaussCtrlModel(GaussCtrlModelConfig(background_color="black"), params=P, device=DEV)
    cfg = GaussCtrlPipelineConfig(edit_prompt="a polar bear", reverse_prompt="a bear", langsam_obj="bear", chunk_size=3, edit_region=edit_region,
                                  synthetic_weights=True)
    pipe = object.__new__(GaussCtrlPipeline)
    torch.nn.Module.__init__(pipe)
    pipe.config, pipe.datamanager, pipe._model, pipe._dev = cfg, SimpleDataManager(cams), model, torch.device(DEV)
    pipe.world_size, pipe.local_rank, pipe.test_mode, pipe._spread_calls, pipe.chunk_size = 1, 0, "val", 0, 3
    pipe.mask_fn = lambda rgb, obj: torch.arange(rgb.shape[1], device=rgb.device)[None, :].expand(rgb.shape[0], -1) < rgb.shape[1] // 2
    pipe.positive_reverse_prompt = "a bear"
    pipe.text_encoder = lambda prompt: torch.zeros(1, 77, 768)
    pipe.image2latent = lambda image: torch.zeros(1, 4, 8, 8, device=DEV)
    pipe.depth2disparity_torch = lambda depth: torch.zeros(3, 64, 64, device=DEV)
    pipe.pipe = types.SimpleNamespace(invert=lambda lat, disp, ctx: lat)
    pipe.render_reverse()
    sel0 = None
    if edit_region == "traced":
        sel0 = model.edit_select.clone()
        assert sel0.dtype == torch.uint8 and sel0.shape == (model.num_points,)
    else:
        assert getattr(model, "edit_select", None) is None
    for t in pipe.datamanager.train_data:
        assert t["mask_image"].shape == (64, 64)
        t["image"] = t["unedited_image"] * 0.5               # a target every pixel of which pulls on the render
    opts = build_optimizers(model)
    cbs = model.get_training_callbacks(TrainingCallbackAttributes(optimizers=opts, grad_scaler=None, pipeline=pipe))
    idx = torch.arange(model.num_points, device=DEV)
    culled = 0
    for step in range(30000, 30005):
        for cb in cbs:
            cb.run_callback_at_location(step, "before_train_iteration")
        pipe.train_iteration(opts, step)
        c = model.config
        if step % c.refine_every == 0:                        # CullCallback's rule, on the parameters it is about to see
            with torch.no_grad():
                culls = (torch.sigmoid(model.opacities) < c.cull_alpha_thresh).squeeze(-1) | (torch.exp(model.scales).max(dim=-1).values > c.cull_scale_thresh)
            idx = idx[~culls]
            culled += int(culls.sum())
        for cb in cbs:
            cb.run_callback_at_location(step, "after_train_iteration")
        assert model.num_points == idx.numel()
    assert culled > 0
    return model, idx, sel0


def test_traced_edit_region_end_to_end():
    """edit_region "traced": every unselected surviving row of all six parameters keeps its initial bits through 5 iterations and a cull,
    selected rows move, model.edit_select follows the cull; the same run with "image" moves unselected rows too (the test can fail).
    Moved: a selected row received compositing weight in some view, so its colour gradient is non-zero wherever the target differs from
    the render, and Adam's first steps move a row by about its learning rate whatever the gradient's size; 5 iterations visit all 3 views."""
    from gaussctrl_amd.ns_compat import Cameras
    P = syn.make_gaussians(2000, seed=4, scale_mean=0.05)
    cams = Cameras(syn.make_cameras(3, seed=12), 60.0, 60.0, 32.0, 32.0, 64, 64)
    init = {k: _t(v) for k, v in P.items()}
    model, idx, sel0 = _edit_run(P, cams, "traced")
    sel = model.edit_select
    assert sel.shape == (model.num_points,) and torch.equal(sel, sel0[idx])
    on = sel.bool()
    assert 0 < int(on.sum()) < model.num_points and 0 < int(sel0.sum()) < sel0.numel()
    for k in ("means", "scales", "quats", "opacities", "features_dc", "features_rest"):
        got, was = getattr(model, k).detach(), init[k][idx]
        assert torch.equal(_bits(got[~on]), _bits(was[~on])), k
        moved = (got[on] != was[on]).reshape(int(on.sum()), -1).any(dim=1)
        print(f"traced: {k}: {int(moved.sum())} of {int(on.sum())} selected rows moved")
        assert float(moved.float().mean()) > 0.5, k
    model2, idx2, _ = _edit_run(P, cams, "image")
    off2 = sel0[idx2] == 0
    for k in ("means", "features_dc"):
        got, was = getattr(model2, k).detach(), init[k][idx2]
        moved = (got[off2] != was[off2]).reshape(int(off2.sum()), -1).any(dim=1)
        print(f"image: {k}: {int(moved.sum())} of {int(off2.sum())} unselected rows moved")
        assert bool(moved.any()), k


# ------------------------------------------------------------------------------------------------------------------ 6. red zones
def _guarded(fn, nbytes, **kw):
    import sys
    from gaussctrl_amd import edit_region, gsplat_ops, train_ops
    with guard(gsplat_ops, train_ops, edit_region, sys.modules[__name__], nbytes=nbytes):
        fn(**kw)


@pytest.mark.parametrize("scene", [TINY, SMALL0], ids=["tiny", "small0"])
def test_guarded_sums(scene):
    """test 1 again with every buffer -- inputs, lists, workspaces, masks, the two sums, the selection -- inside a red-zone arena"""
    _guarded(test_sums_vs_fp64_oracle, 512 << 20, scene=scene, aa=False)


@pytest.mark.parametrize("rows", [1, 5, 1027])
@pytest.mark.parametrize("rf", [1, 3, 4, 45])
def test_guarded_adam_step_rows(rows, rf):
    _guarded(test_adam_step_rows, 64 << 20, rows=rows, rf=rf)
