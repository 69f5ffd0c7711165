"""Crafted tile lists for the compositing kernels alone, and a float64 closed form of their backward per (pixel, list entry) (plain helper,
like _inside_scene.py).

A scene IS the compositing kernels' input: xys [N,2], conics [N,3], colors [N,3], opac [N], extra [N] (a positive "depth"), background [3],
ids_sorted, tile_bins -- float32 values from seeded numpy generators, no projection.  The lists are the helper's own (any (ids, bins) is a
legal input): tile t holds the first LEN[t] splats of a seeded depth order.  Images are at most 3 x 3 tiles with partial tiles right and below.

    deep     44 x 37, 700 splats, opacity 0.005-0.08, sd 1.5-12 px, LEN (256, 257, 513, 1, 255, 512, 700, 700, 0): one, two and three
             backward batches and both sides of each batch edge, an empty and a one-entry tile; no pixel stops (the whole list is replayed),
             nothing exceeds 1 before the clamp
    stop     44 x 37, 300 splats, opacity 0.3-0.95, sd 2-7 px, every list 257 to 300 long; the centres crowd towards the left edge
             (x = W u^3), so pixels end at T_STOP at very different list positions
    opaque   44 x 37, 200 splats in 40 stacks centred (to 0.01 px) on pixels; the even ones are near-opaque (opacity from {0.9, 0.99, 0.9995,
             0.99999}, sd 3-6 px, the two that can reach the cap tend to the front of the depth order), the odd ones translucent (0.004-0.6
             log-uniform, sd 1.5-3 px); colours in [-0.25, 1.5]; LEN (200, 200, 40, 200, 200, 40, 200, 200, 0): araw on both sides of the cap,
             ra up to 1000, pre-clamp rgb on both sides of 1, pixels of alpha exactly 0
    tiny     17 x 9, 3 splats: one full-width and one 1-pixel-wide partial tile (the staging tails)

scene(name, view, own_opac): view > 0 draws another geometry (xys, conics, colors, extra, depth order) for the batched entry points;
opacities and background are view 0's unless own_opac.

Census (census(name), float64; test_composite_vjp_cpu.py asserts the floors) -- measured:
    deep     71 valid pairs per pixel, min T_final 0.033, no pixel stops, largest pre-clamp channel 0.84, 4 tiles with kmax >= 256 (8 splats
             redrawn)
    stop     67 % of the pixels stop early; tile 6 has kmax 121 entries before the end of its list; tile 3's four waves have wmax 204, 275,
             152, 228; 7 tiles with kmax >= 256; 98 faint rows (2 redrawn)
    opaque   10 capped pairs (ra = 1000), 696 pre-clamp channels above 1, 60 pixels of alpha 0, 35 % of the pixels stop, 67 faint rows: non-zero
             rows below 1e-4 of their tensor's largest row under set a, 42 of them in v_xy (24 redrawn)
    tiny     2.9 valid pairs per pixel, 153 pixels

No knife edges -- a condition, not an allowance.  Constants: both precisions use the float32 values of 0.999, 1/255 and 1e-4 that the kernels
compare against (as _inside_scene hands both precisions the float32 camera), so the two differ in arithmetic alone.  For every (pixel, list
entry) up to and including the pixel's stopping entry, in float64: |ln(alpha / ALPHA_MIN)|, |ln(araw / ALPHA_CAP)|, |ln(T (1 - alpha) / T_STOP)|
(valid pairs) and sigma - 0; per pixel |pre-clamp channel - 1|; pixel alpha is 0 exactly or >= 1/255 by construction.  Each distance must be
at least MARGIN = 16 x the largest |float32 - float64| difference of the same quantity on that scene (measured over the pairs within 1 of
the threshold -- the only ones whose decision could move; every other pair's difference is asserted below half its own distance).  A splat that owns a pair
inside the margin gets a new geometry from a generator seeded by (scene, view, splat, round).  Then both precisions take every discrete
decision alike and the GPU tests demand exact final_index.

Reference: pair_backward(sc, cot, dtype, depth, colors, clamp, fault) is SURVEY A.5 per (pixel, entry), vectorised per tile, replayed back
to front from the forward's T_final and final_index (T_k = ((T_final ra_last) ra_..) ra_k, S_k = sum over later entries of c fac), with
the finalize epilogue folded in under `depth` (depth = E / alpha_px, no gradient where alpha_px == 0) and the clamp backward under `clamp`.
Per output it returns the signed sum and the term-wise absolute sum A (every added term replaced by its magnitude: |c T vo|, |S ra vo|,
|T_final ra v_alpha|, |T_final ra bgdot|, |e T vE|, |S3 ra vE|, |T_final ra vd depth / alpha_px|, times the magnitude of the geometric factor,
summed over pixels), and xy_abs = sum over pixels of (|g_x|, |g_y|).  float64 is the reference; float32 rounds after every operation and adds
sequentially (list order inside a pixel, pixel order inside a tile, tile order) and exists only to measure the bars.

Row metric: e = |got_r - ref_r|_2 / |A_r|_2; a row with A_r == 0 must be exactly 0.  BARS[k] = 8 x the worst e of the float32 closed form
against the float64 one over all scenes and cotangent sets (rounded down to two digits; 8 and not the projection tests' 4: the device uses
__expf and a 1-ulp reciprocal where numpy's are correctly rounded, and sums by DPP rows and float atomics in another order).  Measured
(reference_distances(); test_composite_vjp_cpu.test_bar_window asserts 2 x measured <= bar <= 8 x measured):

    v_xy 6.12e-7   v_conic 6.46e-7   v_colors 7.44e-7   v_opacity 6.72e-7   v_extra 7.08e-7 (held to the colours' bar)   xy_abs 6.48e-7 (v_xy's)

FWD_BARS the same way, per pixel: image |got - ref|_2 / (sum_k |c_k|_2 alpha_k T_k + T_final |bg|_2), extra |got - ref| / sum_k |e_k| alpha_k T_k,
final_Ts |got - ref| / T_final.  Measured: image 6.77e-7, extra 1.10e-6, final_Ts 4.18e-6.

Cotangent sets (seeded normal float32): a = v_out, v_alpha (and v_depth where taken); b = v_out only; c = v_alpha only; d = v_depth only.
"""
import numpy as np

TILE = 16
F32, F64 = np.float32, np.float64
ALPHA_CAP, ALPHA_MIN, T_STOP = F32(0.999), F32(1.0) / F32(255.0), F32(1e-4)
KEYS = ("v_xy", "v_conic", "v_colors", "v_opacity")
BARS = {"v_xy": 4.8e-6, "v_conic": 5.1e-6, "v_colors": 5.9e-6, "v_opacity": 5.3e-6}
BARS["v_extra"] = BARS["v_colors"]
BARS["xy_abs"] = BARS["v_xy"]
FWD_BARS = {"image": 5.4e-6, "extra": 8.8e-6, "final_Ts": 3.3e-5}
SPECS = {"deep": dict(W=44, H=37, N=700, seed=13, LEN=(256, 257, 513, 1, 255, 512, 700, 700, 0)),
         "stop": dict(W=44, H=37, N=300, seed=12, LEN=(300, 257, 300, 280, 300, 258, 300, 270, 300)),
         "opaque": dict(W=44, H=37, N=200, seed=26, LEN=(200, 200, 40, 200, 200, 40, 200, 200, 0)),
         "tiny": dict(W=17, H=9, N=3, seed=14, LEN=(3, 2))}
SCENES = tuple(SPECS)
STACKS = 40
MARGIN_FACTOR = 16.0
_CACHE = {}


# ---------------------------------------------------------------------------------------- scenes
def _geometry(name, g, i, stacks):
    """one splat's (x, y, cxx, cxy, cyy) from generator g"""
    sp = SPECS[name]
    W, H = sp["W"], sp["H"]
    if name == "deep":
        x, y, lo, hi = g.uniform(-4, W + 4), g.uniform(-4, H + 4), 1.5, 12.0
    elif name == "stop":
        x, y, lo, hi = W * g.uniform(0, 1) ** 3, g.uniform(-2, H + 2), 2.0, 7.0
    elif name == "opaque":
        cx, cy = stacks[i % STACKS]
        x, y = cx + g.normal(0, 0.01), cy + g.normal(0, 0.01)
        lo, hi = (1.5, 3.0) if i % 2 else (3.0, 6.0)                     # odd: the small translucent ones; even: the near-opaque ones
    else:
        x, y, lo, hi = 8 + g.normal(0, 2), 4 + g.normal(0, 2), 2.0, 5.0
    s1, s2, th = g.uniform(lo, hi), g.uniform(lo, hi), g.uniform(0, np.pi)
    c, s = np.cos(th), np.sin(th)
    a, b = 1.0 / s1 ** 2, 1.0 / s2 ** 2                                  # inverse covariance R diag(a, b) R^T
    return [x, y, a * c * c + b * s * s, (a - b) * c * s, a * s * s + b * c * c]


def _draw(name, view, own_opac):
    sp = SPECS[name]
    N, W, H = sp["N"], sp["W"], sp["H"]
    g = np.random.default_rng([sp["seed"], view])
    go = np.random.default_rng([sp["seed"], 1000 + (view if own_opac else 0)])
    stacks = np.stack([g.integers(3, 41, STACKS), g.integers(3, 34, STACKS)], 1) if name == "opaque" else None
    order = g.permutation(N)
    geo = np.array([_geometry(name, g, i, stacks) for i in range(N)])
    if name == "deep":
        opac, colors = go.uniform(0.005, 0.08, N), g.uniform(0, 0.9, (N, 3))
    elif name == "opaque":
        opac = np.where(np.arange(N) % 2 == 0, go.choice([0.9, 0.99, 0.9995, 0.99999], N), np.exp(go.uniform(np.log(0.004), np.log(0.6), N)))
        colors = g.uniform(-0.25, 1.5, (N, 3))
    else:
        opac, colors = go.uniform(0.3, 0.95, N), g.uniform(0, 0.9, (N, 3))
    # the depth order; in `opaque` the splats that can reach the cap tend to the front, so that pixels reach them before they stop
    if name == "opaque":
        order = np.argsort(g.uniform(size=N) * np.where(opac > 0.999, 0.25, 1.0), kind="stable")
    tx, ty = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    assert len(sp["LEN"]) == tx * ty
    ids = np.concatenate([order[:n] for n in sp["LEN"]]).astype(np.int32)
    ends = np.cumsum(sp["LEN"])
    bins = np.stack([ends - np.array(sp["LEN"]), ends], 1).astype(np.int32)
    return dict(name=name, view=view, W=W, H=H, N=N, tiles=(tx, ty), xys=geo[:, :2].astype(F32), conics=geo[:, 2:].astype(F32),
                colors=colors.astype(F32), opac=opac.astype(F32), extra=g.uniform(0.5, 5.0, N).astype(F32),
                background=go.uniform(0, 0.9, 3).astype(F32), ids_sorted=ids, tile_bins=bins, stacks=stacks)


def scene(name, view=0, own_opac=False):
    """the scene (cached: do not write to its arrays) after the redraw of every splat that owns a knife-edge pair; "redrawn" counts them"""
    key = ("scene", name, view, own_opac and view > 0)
    if key not in _CACHE:
        sc = _draw(name, view, own_opac)
        sc["redrawn"] = 0
        for rnd in range(1, 200):
            owners = knife_edges(sc)["owners"]
            if not len(owners):
                break
            for i in owners:
                g = np.random.default_rng([SPECS[name]["seed"], view, int(i), rnd])
                geo = _geometry(name, g, int(i), sc["stacks"])
                sc["xys"][i], sc["conics"][i] = np.array(geo[:2], F32), np.array(geo[2:], F32)
            sc["redrawn"] += len(owners)
        else:
            raise AssertionError(f"{name}: the redraw of knife-edge splats did not end")
        _CACHE[key] = sc
    return _CACHE[key]


def colors_nd(sc, C):
    """seeded colours [N, C] for the N-channel kernels (C = 3: the scene's own) and their background [C]"""
    if C == 3:
        return sc["colors"], sc["background"]
    g = np.random.default_rng([SPECS[sc["name"]]["seed"], 77, C])
    lo, hi = (-0.25, 1.5) if sc["name"] == "opaque" else (0.0, 0.9)
    return g.uniform(lo, hi, (sc["N"], C)).astype(F32), g.uniform(0, 0.9, C).astype(F32)


def cotangents(sc, cset, C=3, depth=False):
    """{"v_out" [H,W,C], "v_alpha" [H,W] | None, "v_depth" [H,W] | None}; the sets share their draws.  v_out is zeros where the set has none
    (the kernels always read it)."""
    g = np.random.default_rng([SPECS[sc["name"]]["seed"], 500 + sc["view"], C])
    H, W = sc["H"], sc["W"]
    vo, va, vd = g.normal(size=(H, W, C)).astype(F32), g.normal(size=(H, W)).astype(F32), g.normal(size=(H, W)).astype(F32)
    return dict(v_out=vo if cset in "ab" else np.zeros_like(vo), v_alpha=va if cset in "ac" else None,
                v_depth=vd if (cset == "a" and depth) or cset == "d" else None)


# ---------------------------------------------------------------------------------------- the forward per (pixel, entry)
def _exp(x, dt):
    return np.exp(x.astype(F64)).astype(dt)          # float32: the correctly rounded value, the same on every machine


def _tile_pixels(sc, t):
    tx, ty = sc["tiles"]
    h0, w0 = (t // tx) * TILE, (t % tx) * TILE
    py, px = np.meshgrid(np.arange(h0, min(h0 + TILE, sc["H"])), np.arange(w0, min(w0 + TILE, sc["W"])), indexing="ij")
    return py.reshape(-1), px.reshape(-1)


def tile_pairs(sc, t, dt):
    """every (pixel, entry) of tile t in precision dt: [P, L] arrays (P pixels row-major, L list entries front to back), or None (empty)"""
    s, e = (int(v) for v in sc["tile_bins"][t])
    if e <= s:
        return None
    gid = sc["ids_sorted"][s:e].astype(np.int64)
    py, px = _tile_pixels(sc, t)
    cn = sc["conics"][gid].astype(dt)
    dx = sc["xys"][gid, 0].astype(dt)[None, :] - px.astype(dt)[:, None]
    dy = sc["xys"][gid, 1].astype(dt)[None, :] - py.astype(dt)[:, None]
    sigma = dt(0.5) * (cn[:, 0] * dx * dx + cn[:, 2] * dy * dy) + cn[:, 1] * dx * dy
    vis = _exp(-sigma, dt)
    opac = sc["opac"][gid].astype(dt)
    araw = opac[None, :] * vis
    alpha = np.minimum(dt(ALPHA_CAP), araw)
    valid = (sigma >= 0) & (alpha >= dt(ALPHA_MIN))
    one_m = dt(1) - np.where(valid, alpha, dt(0))
    T_incl = np.cumprod(one_m, axis=1, dtype=dt)
    T_excl = np.concatenate([np.ones_like(T_incl[:, :1]), T_incl[:, :-1]], 1)
    stop = valid & (T_incl <= dt(T_STOP))
    nstop = np.cumsum(stop, axis=1)
    contrib = valid & (nstop == 0)
    decided = (nstop - stop) == 0                               # up to and including the stopping entry: where a decision is taken
    T_final = np.cumprod(np.where(contrib, one_m, dt(1)), axis=1, dtype=dt)[:, -1]
    kk = np.arange(s, e, dtype=np.int32)[None, :]
    last = np.where(contrib, kk, 0).max(1).astype(np.int32)
    return dict(gid=gid, py=py, px=px, s=s, dx=dx, dy=dy, sigma=sigma, vis=vis, araw=araw, alpha=alpha, valid=valid, contrib=contrib,
                decided=decided, T_excl=T_excl, T_incl=T_incl, T_final=T_final, last=last, opac=opac, cn=cn,
                stopped=nstop[:, -1] > 0)


def _lsum(x, dt):          # over the list, front to back
    return x.sum(1) if dt is F64 else np.cumsum(x, axis=1, dtype=dt)[:, -1]


def _psum(x, dt):          # over the pixels of a tile, in pixel order
    return x.sum(0) if dt is F64 else np.cumsum(x, axis=0, dtype=dt)[-1]


def forward(sc, dt=F64, colors=None, background=None):
    """image [H,W,C] (before any clamp), final_Ts, final_index, extra [H,W] (E, not finalized), and the metric's denominators"""
    key = ("fwd", sc["name"], sc["view"], id(sc), dt, None if colors is None else colors.shape[1])
    if key in _CACHE:
        return _CACHE[key]
    col = (sc["colors"] if colors is None else colors).astype(dt)
    bg = (sc["background"] if background is None else background).astype(dt)
    H, W, C = sc["H"], sc["W"], col.shape[1]
    img, fT, fi = np.zeros((H, W, C), dt), np.ones((H, W), dt), np.zeros((H, W), np.int32)
    E, den_img, den_E = np.zeros((H, W), dt), np.zeros((H, W), dt), np.zeros((H, W), dt)
    stopped, nvalid = np.zeros((H, W), bool), np.zeros((H, W), np.int64)
    for t in range(len(sc["tile_bins"])):
        p = tile_pairs(sc, t, dt)
        if p is None:
            continue
        w = np.where(p["contrib"], p["alpha"] * p["T_excl"], dt(0))
        for c in range(C):
            img[p["py"], p["px"], c] = _lsum(w * col[p["gid"], c][None, :], dt)
        ex = sc["extra"][p["gid"]].astype(dt)
        E[p["py"], p["px"]] = _lsum(w * ex[None, :], dt)
        den_img[p["py"], p["px"]] = (w * np.linalg.norm(col[p["gid"]].astype(F64), axis=1)[None, :]).sum(1)
        den_E[p["py"], p["px"]] = (w * np.abs(ex)[None, :]).sum(1)
        fT[p["py"], p["px"]], fi[p["py"], p["px"]] = p["T_final"], p["last"]
        stopped[p["py"], p["px"]], nvalid[p["py"], p["px"]] = p["stopped"], p["contrib"].sum(1)
    img = img + fT[..., None] * bg
    out = dict(image=img, final_Ts=fT, final_index=fi, extra=E, stopped=stopped, nvalid=nvalid,
               den_image=den_img.astype(F64) + fT.astype(F64) * np.linalg.norm(bg.astype(F64)), den_extra=den_E.astype(F64))
    _CACHE[key] = out
    return out


def finalize_depth(E, fT):
    """gc_raster_finalize's depth image: E / alpha_px, 1000 where alpha_px == 0 (in the precision of its arguments)"""
    a = 1 - fT
    return np.where(a > 0, E / np.where(a > 0, a, 1), 1000).astype(E.dtype)


def forward_errors(got, ref):
    """{image, extra, final_Ts: worst per-pixel error of `got` (arrays; missing keys skipped) against forward(..., F64)}; a pixel whose
    denominator is 0 must agree exactly"""
    out = {}
    for k, den in (("image", ref["den_image"]), ("extra", ref["den_extra"]), ("final_Ts", ref["final_Ts"].astype(F64))):
        if got.get(k) is None:
            continue
        g = np.asarray(got[k], F64)
        assert np.isfinite(g).all(), k
        d = np.abs(g - ref[k])
        d = np.sqrt((d * d).sum(-1)) if d.ndim == 3 else d
        live = den > 0
        assert np.all(d[~live] == 0), f"{k}: a pixel nothing reaches is not exact"
        out[k] = float((d[live] / den[live]).max()) if live.any() else 0.0
    return out


def forward_distances():
    if "fdist" not in _CACHE:
        worst = dict.fromkeys(FWD_BARS, 0.0)
        for name in SCENES:
            sc = scene(name)
            for k, v in forward_errors(forward(sc, F32), forward(sc, F64)).items():
                worst[k] = max(worst[k], v)
        _CACHE["fdist"] = worst
    return _CACHE["fdist"]


# ---------------------------------------------------------------------------------------- knife edges
def knife_edges(sc):
    """margins (16 x the float32-float64 difference of each quantity), the smallest float64 distance of each, and the splats that own a pair
    (or a pixel) inside its margin"""
    diff = dict.fromkeys(("alpha", "cap", "stop", "sigma", "clamp"), 0.0)
    rows = []
    far = 0.0
    for t in range(len(sc["tile_bins"])):
        p64, p32 = tile_pairs(sc, t, F64), tile_pairs(sc, t, F32)
        if p64 is None:
            continue
        dec = p64["decided"]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = {"alpha": np.log(p64["alpha"] / F64(ALPHA_MIN)), "cap": np.log(p64["araw"] / F64(ALPHA_CAP)),
                 "stop": np.log(p64["T_incl"] / F64(T_STOP)), "sigma": p64["sigma"]}
            d = {"alpha": np.abs(np.log(p32["alpha"].astype(F64)) - np.log(p64["alpha"])),
                 "cap": np.abs(np.log(p32["araw"].astype(F64)) - np.log(p64["araw"])),
                 "stop": np.abs(np.log(p32["T_incl"].astype(F64)) - np.log(p64["T_incl"])),
                 "sigma": np.abs(p32["sigma"].astype(F64) - p64["sigma"])}
        use = {"alpha": dec, "cap": dec, "stop": dec & p64["valid"], "sigma": dec}
        for k in q:
            near = use[k] & (np.abs(q[k]) <= 1)
            if near.any():
                diff[k] = max(diff[k], float(d[k][near].max()))
            rest = use[k] & ~near & np.isfinite(q[k]) & np.isfinite(d[k])
            if rest.any():
                far = max(far, float((d[k][rest] / np.abs(q[k][rest])).max()))
        rows.append((p64, q, use))
    f64, f32 = (_forward_nocache(sc, dt) for dt in (F64, F32))
    diff["clamp"] = float(np.abs(f32.astype(F64) - f64).max())
    margin = {k: MARGIN_FACTOR * v for k, v in diff.items()}
    dist = dict.fromkeys(diff, np.inf)
    owners = set()
    for p64, q, use in rows:
        for k in q:
            a = np.where(use[k], np.abs(q[k]), np.inf)
            if k == "sigma":
                a = np.where(p64["sigma"] == 0, np.inf, a)              # exactly 0 by construction is fine
            dist[k] = min(dist[k], float(a.min()))
            owners.update(p64["gid"][np.nonzero((a < margin[k]).any(0))[0]].tolist())
    c = np.abs(f64 - 1.0)
    dist["clamp"] = float(c.min())
    for i, j, _ in zip(*np.nonzero(c < margin["clamp"])):                 # a pixel inside: its front-most contributing splat moves
        t = (i // TILE) * sc["tiles"][0] + j // TILE
        p = tile_pairs(sc, t, F64)
        row = int(np.nonzero((p["py"] == i) & (p["px"] == j))[0][0])
        owners.add(int(p["gid"][int(np.argmax(p["contrib"][row]))]))
    return dict(margin=margin, dist=dist, owners=sorted(owners), far=far)


def _forward_nocache(sc, dt):
    col, bg = sc["colors"].astype(dt), sc["background"].astype(dt)
    img = np.zeros((sc["H"], sc["W"], 3), dt)
    for t in range(len(sc["tile_bins"])):
        p = tile_pairs(sc, t, dt)
        if p is None:
            img[_tile_pixels(sc, t)] = bg
            continue
        w = np.where(p["contrib"], p["alpha"] * p["T_excl"], dt(0))
        for c in range(3):
            img[p["py"], p["px"], c] = _lsum(w * col[p["gid"], c][None, :], dt) + p["T_final"] * bg[c]
    return img


# ---------------------------------------------------------------------------------------- the backward per (pixel, entry)
FAULTS = ("batch_edge", "cap_passes", "no_bgdot", "t_drift", "s_after")


def batch_edge_target(sc):
    """(tile, local list position kmax - 256, 8x8 block, that weight) of fault (i): over the tiles whose backward has a second batch, the block in which
    the entry at the batch edge composites with the least total weight sum alpha T (but at one pixel at least) -- the loss that is hardest
    to see"""
    f = forward(sc, F64)
    best = None
    for t in range(len(sc["tile_bins"])):
        p = tile_pairs(sc, t, F64)
        if p is None:
            continue
        kmax = int(f["final_index"][p["py"], p["px"]].max()) - p["s"]
        if kmax >= 256:
            blk = ((p["py"] % TILE) >= 8) * 2 + ((p["px"] % TILE) >= 8)
            for b in range(4):
                n = float(np.where(p["contrib"], p["alpha"] * p["T_excl"], 0.0)[blk == b, kmax - 256].sum())
                if n and (best is None or n < best[0]):
                    best = (n, t, kmax - 256, b)
    return None if best is None else best[1:] + best[:1]


def _rev_cum(x, dt, op):          # inclusive, from the back of the list, sequential
    return op(x[:, ::-1], axis=1, dtype=dt)[:, ::-1]


def pair_backward(sc, cot, dt=F64, depth=False, colors=None, background=None, clamp=False, fault=None):
    """-> {"v_xy" | "v_conic" | "v_colors" | "v_opacity" [| "v_extra"]: (signed sum, A), "xy_abs": [N, 2]} as float64 arrays"""
    col = (sc["colors"] if colors is None else colors).astype(dt)
    bg = (sc["background"] if background is None else background).astype(dt)
    N, C = sc["N"], col.shape[1]
    fwd = forward(sc, dt, colors, background)
    v_out = cot["v_out"].astype(dt)
    if clamp:
        v_out = np.where(fwd["image"] <= 1, v_out, dt(0))
    v_al = None if cot["v_alpha"] is None else cot["v_alpha"].astype(dt)
    v_dp = cot["v_depth"].astype(dt) if depth and cot["v_depth"] is not None else None
    dep_img = finalize_depth(fwd["extra"], fwd["final_Ts"]) if depth else None
    shapes = {"v_xy": 2, "v_conic": 3, "v_colors": C, "v_opacity": 1, **({"v_extra": 1} if depth else {}), "xy_abs": 2}
    S = {k: np.zeros((N, w), dt) for k, w in shapes.items()}
    A = {k: np.zeros((N, w), F64) for k, w in shapes.items() if k != "xy_abs"}
    edge = batch_edge_target(sc) if fault == "batch_edge" else None
    for t in range(len(sc["tile_bins"])):
        p = tile_pairs(sc, t, dt)
        if p is None:
            continue
        gid, py, px = p["gid"], p["py"], p["px"]
        Tf = fwd["final_Ts"][py, px]
        con = p["valid"] & ((np.arange(p["s"], p["s"] + len(gid))[None, :]) <= fwd["final_index"][py, px][:, None])
        keep = np.ones(con.shape, bool)          # fault (i): the entry's partials of one block are lost; the replay of T and S goes on
        if edge is not None and edge[0] == t:
            keep[(((py % TILE) >= 8) * 2 + ((px % TILE) >= 8)) == edge[2], edge[1]] = False
        ra = np.where(con, dt(1) / (dt(1) - np.where(con, p["alpha"], dt(0))), dt(1))
        Tk = np.cumprod(np.concatenate([Tf[:, None], ra[:, ::-1]], 1), axis=1, dtype=dt)[:, :0:-1]
        if fault == "t_drift":
            back = np.maximum(fwd["final_index"][py, px][:, None] - np.arange(p["s"], p["s"] + len(gid))[None, :], 0)
            Tk = Tk * (1 + 1e-4 * back / 256.0)
        fac = np.where(con, p["alpha"] * Tk, dt(0))
        vo = v_out[py, px]                                               # [P, C]
        voa = np.zeros(len(py), dt) if v_al is None else v_al[py, px]
        bgdot = np.zeros(len(py), dt)
        for c in range(C):
            bgdot = bgdot + bg[c] * vo[:, c]
        if fault == "no_bgdot":
            bgdot = np.zeros_like(bgdot)
        va, Ava = np.zeros_like(fac), np.zeros(fac.shape, F64)
        chans = [(col[gid, c], vo[:, c], "v_colors", c) for c in range(C)]
        d_alpha = None
        if v_dp is not None:
            apx = dt(1) - Tf
            pos = apx > 0
            safe = np.where(pos, apx, dt(1))
            vE = np.where(pos, v_dp[py, px] / safe, dt(0))
            d_alpha = np.where(pos, -v_dp[py, px] * dep_img[py, px] / safe, dt(0))
            chans.append((sc["extra"][gid].astype(dt), vE, "v_extra", 0))
        elif depth:
            chans.append((sc["extra"][gid].astype(dt), np.zeros(len(py), dt), "v_extra", 0))
        for cv, vc, key, c in chans:
            cf = cv[None, :] * fac
            Sin = _rev_cum(cf, dt, np.cumsum)
            Sex = Sin if fault == "s_after" else np.concatenate([Sin[:, 1:], np.zeros_like(Sin[:, :1])], 1)
            t1, t2 = cv[None, :] * Tk * vc[:, None], Sex * ra * vc[:, None]
            va = va + (cv[None, :] * Tk - Sex * ra) * vc[:, None]
            Ava += np.abs(t1.astype(F64)) + np.abs(t2.astype(F64))
            g = np.where(keep, fac * vc[:, None], dt(0))
            S[key][gid, c] += _psum(g, dt)
            A[key][gid, c] += np.abs(g.astype(F64)).sum(0)
        Tra = Tf[:, None] * ra
        va = va + Tra * voa[:, None]
        va = va + -Tra * bgdot[:, None]
        Ava += np.abs((Tra * voa[:, None]).astype(F64)) + np.abs((Tra * bgdot[:, None]).astype(F64))
        if d_alpha is not None:
            va = va + Tra * d_alpha[:, None]
            Ava += np.abs((Tra * d_alpha[:, None]).astype(F64))
        passes = keep & (con if fault == "cap_passes" else con & ~(p["araw"] > dt(ALPHA_CAP)))
        vav = np.where(passes, p["vis"] * va, dt(0))                     # the opacity partial
        Avav = np.where(passes, p["vis"].astype(F64) * Ava, 0.0)
        vs, Avs = -p["opac"][None, :] * vav, p["opac"].astype(F64)[None, :] * Avav
        dx, dy, cn = p["dx"], p["dy"], p["cn"]
        gx, gy = vs * (cn[None, :, 0] * dx + cn[None, :, 1] * dy), vs * (cn[None, :, 1] * dx + cn[None, :, 2] * dy)
        terms = {("v_opacity", 0): (vav, 1.0), ("v_conic", 0): (dt(0.5) * vs * dx * dx, 0.5 * dx * dx), ("v_conic", 1): (vs * dx * dy, dx * dy),
                 ("v_conic", 2): (dt(0.5) * vs * dy * dy, 0.5 * dy * dy), ("v_xy", 0): (gx, cn[None, :, 0] * dx + cn[None, :, 1] * dy),
                 ("v_xy", 1): (gy, cn[None, :, 1] * dx + cn[None, :, 2] * dy)}
        for (key, c), (g, geo) in terms.items():
            S[key][gid, c] += _psum(g, dt)
            A[key][gid, c] += ((Avav if key == "v_opacity" else Avs) * np.abs(np.asarray(geo, F64))).sum(0)
        S["xy_abs"][gid, 0] += _psum(np.abs(gx), dt)
        S["xy_abs"][gid, 1] += _psum(np.abs(gy), dt)
    out = {k: (S[k].astype(F64), A[k]) for k in A}
    out["xy_abs"] = S["xy_abs"].astype(F64)
    return out


def reference(sc, cset, depth=False, C=3, clamp=False, dt=F64):
    """pair_backward of a scene under a cotangent set, cached"""
    key = ("ref", sc["name"], sc["view"], id(sc), cset, depth, C, clamp, dt)
    if key not in _CACHE:
        col, bg = colors_nd(sc, C)
        _CACHE[key] = pair_backward(sc, cotangents(sc, cset, C, depth), dt, depth, col, bg, clamp)
    return _CACHE[key]


def _rows(a):
    a = np.asarray(a, F64)
    return a.reshape(a.shape[0], -1)


def row_errors(got, ref, A, slack=None, rows=None):
    """worst e = |got_r - ref_r|_2 / |A_r|_2 over the rows with A_r != 0 (of `rows`, a boolean mask, if given); the others must be exactly 0.
    slack [rows]: an absolute allowance per row (accumulation onto a non-zero buffer).  -> (worst e, rows compared)"""
    d = np.linalg.norm(_rows(got) - _rows(ref), axis=1)
    if slack is not None:
        d = np.maximum(d - slack, 0.0)
    den = np.linalg.norm(_rows(A), axis=1)
    live = den > 0
    assert np.all(d[~live] == 0), "a row no term reaches is not exactly zero"
    if rows is not None:
        live = live & rows
    return (float((d[live] / den[live]).max()) if live.any() else 0.0), int(live.sum())


def faint_rows(sc, ref):
    """{key: mask of the non-zero rows whose reference gradient is below 1e-4 of their tensor's largest row}"""
    out = {}
    for k in KEYS:
        n = np.linalg.norm(_rows(ref[k][0]), axis=1)
        out[k] = (n > 0) & (n < 1e-4 * n.max())
    return out


def reference_distances():
    """worst row error of the float32 closed form against the float64 one per output, over every scene and cotangent set (depth taken under
    a and d): what BARS is eight times of"""
    if "dist" not in _CACHE:
        worst = dict.fromkeys(KEYS + ("v_extra", "xy_abs"), 0.0)
        for name in SCENES:
            sc = scene(name)
            for cset, depth, clamp in (("a", True, False), ("a", False, True), ("b", False, False), ("c", False, False), ("d", True, False)):
                r64, r32 = (reference(sc, cset, depth, 3, clamp, dt) for dt in (F64, F32))
                for k in r64:
                    if k == "xy_abs":
                        worst[k] = max(worst[k], row_errors(r32[k], r64[k], r64["v_xy"][1])[0])
                    else:
                        worst[k] = max(worst[k], row_errors(r32[k][0], r64[k][0], r64[k][1])[0])
        _CACHE["dist"] = worst
    return _CACHE["dist"]


# ---------------------------------------------------------------------------------------- census
def census(name):
    if ("census", name) not in _CACHE:
        sc = scene(name)
        f = forward(sc, F64)
        c = dict(redrawn=sc["redrawn"], pixels=sc["H"] * sc["W"], valid_per_pixel=float(f["nvalid"].mean()), min_T=float(f["final_Ts"].min()),
                 stopped=float(f["stopped"].mean()), max_preclamp=float(f["image"].max()), above_one=int((f["image"] > 1).sum()),
                 alpha_zero=int((f["final_Ts"] == 1).sum()), two_batch_tiles=0, kmax_before_end=0, wmax_span=0, capped=0, ra_over_100=0)
        for t in range(len(sc["tile_bins"])):
            p = tile_pairs(sc, t, F64)
            if p is None:
                continue
            local = np.where(p["contrib"].any(1), p["last"] - p["s"], -1)          # final_index within the list; nothing composited: -1
            kmax = int(local.max())
            c["two_batch_tiles"] += kmax >= 256
            c["kmax_before_end"] = max(c["kmax_before_end"], len(p["gid"]) - 1 - kmax)
            blk = ((p["py"] % TILE) >= 8) * 2 + ((p["px"] % TILE) >= 8)
            if len(set(blk.tolist())) == 4:
                w = [int(local[blk == b].max()) for b in range(4)]
                c["wmax_span"] = max(c["wmax_span"], max(w) - min(w))
            c["capped"] += int((p["contrib"] & (p["araw"] > F64(ALPHA_CAP))).sum())
            c["ra_over_100"] += int((p["contrib"] & (p["alpha"] > 0.99)).sum())
        faint = faint_rows(sc, reference(sc, "a"))
        c["faint"] = int(np.any(list(faint.values()), axis=0).sum())
        c["faint_xy"] = int(faint["v_xy"].sum())
        _CACHE[("census", name)] = c
    return _CACHE[("census", name)]
