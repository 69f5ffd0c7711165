"""The distortion map of include/ext/gaussctrl_distort.h on the crafted tile lists of _composite_scene.py, in closed form: float64 forward
(distort, wt) and backward per (pixel, list entry) (plain helper, like _composite_scene.py, on which it builds).

The scenes deep, stop, opaque and tiny are taken as they are (their knife-edge margins cover every discrete decision this feature takes: it
takes none of its own); sc["extra"] is the per-Gaussian depth z, uniform in [0.5, 5).  Depth maps: MODES = (0, 1); mode 1 with NEAR = 0.2
and FAR = 100, the operator layer's defaults, in their float32 values for both precisions (as the compositing constants are).

Forward per pixel, over the entries the compositing forward composites (w = alpha T, T in front of the entry, t = m(z)):
    A_i = 1 - T_i,  B_i = sum_{j<i} w_j t_j,  distort = 2 sum_i w_i (t_i A_i - B_i),  wt = sum_i w_i t_i
Backward: replayed back to front from the forward's T_final and final_index, the way _composite_scene.pair_backward does it
(T_k = ((T_final ra_last) ra_..) ra_k), carrying the suffix sums S, Bs, R, with B_i = (wt - Bs_i) - w_i t_i:
    dD/dw = 2 [(t A - B) + (Bs - t S)],  dD/dt = 2 w (A - S),  dD/dalpha = T dD/dw - R ra
v_alpha = g dD/dalpha goes through the compositing tail (a capped alpha passes nothing) to v_xy, v_conic, v_opacity; v_depths takes
g dD/dt m'(z), cap or not.  Per output row the signed sum and the term-wise absolute sum A: every added term replaced by its magnitude --
|t A|, |B|, |Bs|, |t S| in dD/dw (and through it in R), |T dD/dw| and |R ra| in dD/dalpha, |A| and |S| in dD/dt -- each times the magnitude
of its geometric factor, summed over pixels.  float64 is the reference; float32 rounds after every operation and adds sequentially (list
order inside a pixel, pixel order inside a tile, tile order) and exists only to measure the bars.

Row metric: e = |got_r - ref_r|_2 / |A_r|_2 (cs.row_errors); a row with A_r == 0 must be exactly 0.  Forward metric per pixel:
|got - ref| / (2 sum_i w_i (|t_i A_i| + |B_i|)) for distort, / sum_i |w_i t_i| for wt; a pixel whose sum is 0 must agree exactly.
BARS / FWD_BARS = 8 x the worst e of the float32 closed form against the float64 one over the four scenes, both depth maps and the two
cotangent sets, rounded down to two digits (8 as in _composite_scene: the device uses __expf and a 1-ulp reciprocal and sums by DPP rows and
float atomics in another order).  Measured (reference_distances() / forward_distances(); test_distort_cpu.test_bar_window asserts
2 x measured <= bar <= 8 x measured):

    v_xy 2.32e-7   v_conic 2.41e-7   v_opacity 2.49e-7   v_depths 8.64e-7        distort 2.12e-6   wt 1.10e-6

Cotangent sets (seeded float32): a = normal v_distort; b = uniform in [0.5, 1.5) (one sign, as a mean over the map hands down).

MUTANTS, in the manner of cs.FAULTS: no_r (R dropped from dD/dalpha), s_after (S taken after its update), b_wrong (B taken from the
suffix sum, the running sum of the wrong direction), no_dm (m'(z) missing from v_depths; mode 1 only), cap_passes (a capped pair passes
the alpha gradient).
"""
import numpy as np

import _composite_scene as cs

F32, F64 = np.float32, np.float64
MODES = (0, 1)
NEAR, FAR = F32(0.2), F32(100.0)
KEYS = ("v_xy", "v_conic", "v_opacity", "v_depths")
WIDTH = {"v_xy": 2, "v_conic": 3, "v_opacity": 1, "v_depths": 1}
BARS = {"v_xy": 1.8e-6, "v_conic": 1.9e-6, "v_opacity": 1.9e-6, "v_depths": 6.9e-6}
FWD_BARS = {"distort": 1.6e-5, "wt": 8.8e-6}
CSETS = "ab"
MUTANTS = ("no_r", "s_after", "b_wrong", "no_dm", "cap_passes")
_CACHE = {}


def mapped(z, mode, dt):
    """(t, m'(z)) of depths z in precision dt, the operations in the header's order"""
    z = z.astype(dt)
    if mode == 0:
        return z, np.ones_like(z)
    near, far = dt(NEAR), dt(FAR)
    span = far - near
    return (far * (z - near)) / (span * z), (far * near) / (span * (z * z))


def cotangent(sc, cset):
    """v_distort [H, W] float32"""
    g = np.random.default_rng([cs.SPECS[sc["name"]]["seed"], 900 + sc["view"]])
    n, u = g.normal(size=(sc["H"], sc["W"])).astype(F32), g.uniform(0.5, 1.5, (sc["H"], sc["W"])).astype(F32)
    return n if cset == "a" else u


def _excl(x):          # inclusive running sums along the list -> exclusive ones (front to back)
    return np.concatenate([np.zeros_like(x[:, :1]), x[:, :-1]], 1)


def _excl_back(x):     # the same for sums that run from the back
    return np.concatenate([x[:, 1:], np.zeros_like(x[:, :1])], 1)


def pixel_distort(alpha, t):
    """distort of ONE pixel from the alphas and mapped depths of its composited entries (float64, front to back): the definition, written
    as a loop -- what the central differences of test_distort_cpu.py perturb"""
    T, B, D = 1.0, 0.0, 0.0
    for a, ti in zip(alpha, t):
        w = a * T
        D += 2.0 * w * (ti * (1.0 - T) - B)
        B += w * ti
        T *= 1.0 - a
    return D


def forward(sc, mode, dt=F64):
    """{distort, wt [H, W] in dt; den_distort, den_wt: the metric's per-pixel term-wise sums (float64)}"""
    key = ("fwd", sc["name"], sc["view"], id(sc), mode, dt)
    if key in _CACHE:
        return _CACHE[key]
    H, W = sc["H"], sc["W"]
    out = dict(distort=np.zeros((H, W), dt), wt=np.zeros((H, W), dt), den_distort=np.zeros((H, W), F64), den_wt=np.zeros((H, W), F64))
    for tl in range(len(sc["tile_bins"])):
        p = cs.tile_pairs(sc, tl, dt)
        if p is None:
            continue
        t, _ = mapped(sc["extra"][p["gid"]], mode, dt)
        w = np.where(p["contrib"], p["alpha"] * p["T_excl"], dt(0))
        A = dt(1) - p["T_excl"]
        wt_i = w * t[None, :]
        B = _excl(np.cumsum(wt_i, axis=1, dtype=dt))
        tA = t[None, :] * A
        out["distort"][p["py"], p["px"]] = np.cumsum(dt(2) * w * (tA - B), axis=1, dtype=dt)[:, -1]
        out["wt"][p["py"], p["px"]] = np.cumsum(wt_i, axis=1, dtype=dt)[:, -1]
        w64 = w.astype(F64)
        out["den_distort"][p["py"], p["px"]] = (2 * w64 * (np.abs(tA.astype(F64)) + np.abs(B.astype(F64)))).sum(1)
        out["den_wt"][p["py"], p["px"]] = np.abs(wt_i.astype(F64)).sum(1)
    _CACHE[key] = out
    return out


def forward_errors(got, ref):
    """{distort, wt: worst per-pixel error of `got` against forward(..., F64)}; a pixel whose term-wise sum is 0 must agree exactly"""
    out = {}
    for k in ("distort", "wt"):
        g = np.asarray(got[k], F64)
        assert np.isfinite(g).all(), k
        d, den = np.abs(g - ref[k]), ref["den_" + k]
        live = den > 0
        assert np.all(d[~live] == 0), f"{k}: a pixel nothing reaches is not exact"
        out[k] = float((d[live] / den[live]).max()) if live.any() else 0.0
    return out


def pair_terms(sc, tl, mode, dt=F64, fault=None):
    """the backward of tile tl per (pixel, entry), [P, L] arrays in dt: con (the entries the replay visits), Tk, fac = w, ra, dw, dtt, da
    and the term-wise magnitudes Ada, Adt (float64); t, dm [L]; p = cs.tile_pairs.  None for an empty tile"""
    p = cs.tile_pairs(sc, tl, dt)
    if p is None:
        return None
    fwd, mine = cs.forward(sc, dt), forward(sc, mode, dt)
    py, px, gid = p["py"], p["px"], p["gid"]
    t, dm = mapped(sc["extra"][gid], mode, dt)
    if fault == "no_dm":
        dm = np.ones_like(dm)
    Tf, wtp = fwd["final_Ts"][py, px], mine["wt"][py, px][:, None]
    con = p["valid"] & ((np.arange(p["s"], p["s"] + len(gid))[None, :]) <= fwd["final_index"][py, px][:, None])
    ra = np.where(con, dt(1) / (dt(1) - np.where(con, p["alpha"], dt(0))), dt(1))
    Tk = np.cumprod(np.concatenate([Tf[:, None], ra[:, ::-1]], 1), axis=1, dtype=dt)[:, :0:-1]
    fac = np.where(con, p["alpha"] * Tk, dt(0))
    tt = t[None, :]
    A = dt(1) - Tk
    wti = fac * tt
    S_in, Bs_in = cs._rev_cum(fac, dt, np.cumsum), cs._rev_cum(wti, dt, np.cumsum)
    S = S_in if fault == "s_after" else _excl_back(S_in)
    Bs = _excl_back(Bs_in)
    B = Bs if fault == "b_wrong" else (wtp - Bs) - wti
    tA, tS = tt * A, tt * S
    dw = dt(2) * ((tA - B) + (Bs - tS))
    dtt = dt(2) * fac * (A - S)
    R = _excl_back(cs._rev_cum(fac * dw, dt, np.cumsum))
    if fault == "no_r":
        R = np.zeros_like(R)
    TdW, Rra = Tk * dw, R * ra
    da = TdW - Rra
    a64 = lambda x: np.abs(x.astype(F64))
    Adw = 2 * (a64(tA) + a64(B) + a64(Bs) + a64(tS))
    AR = _excl_back(np.cumsum((a64(fac) * Adw)[:, ::-1], axis=1)[:, ::-1])
    Ada = a64(Tk) * Adw + AR * a64(ra)
    Adt = 2 * a64(fac) * (a64(A) + a64(S))
    return dict(p=p, t=t, dm=dm, con=con, Tk=Tk, fac=fac, ra=ra, dw=dw, dtt=dtt, da=da, Ada=Ada, Adt=Adt)


def pair_backward(sc, v_distort, mode, dt=F64, fault=None):
    """-> {"v_xy" | "v_conic" | "v_opacity" | "v_depths": (signed sum, A)} as float64 arrays [N, w]"""
    N = sc["N"]
    S = {k: np.zeros((N, w), dt) for k, w in WIDTH.items()}
    A = {k: np.zeros((N, w), F64) for k, w in WIDTH.items()}
    vd = v_distort.astype(dt)
    for tl in range(len(sc["tile_bins"])):
        q = pair_terms(sc, tl, mode, dt, fault)
        if q is None:
            continue
        p, con = q["p"], q["con"]
        gid = p["gid"]
        g = vd[p["py"], p["px"]][:, None]
        ag = np.abs(g.astype(F64))
        va, Ava = g * q["da"], ag * q["Ada"]
        gd = np.where(con, g * q["dtt"] * q["dm"][None, :], dt(0))
        S["v_depths"][gid, 0] += cs._psum(gd, dt)
        A["v_depths"][gid, 0] += np.where(con, ag * q["Adt"] * np.abs(q["dm"].astype(F64))[None, :], 0.0).sum(0)
        passes = con if fault == "cap_passes" else con & ~(p["araw"] > dt(cs.ALPHA_CAP))
        vav = np.where(passes, p["vis"] * va, dt(0))                     # the opacity partial
        Avav = np.where(passes, p["vis"].astype(F64) * Ava, 0.0)
        vs, Avs = -p["opac"][None, :] * vav, p["opac"].astype(F64)[None, :] * Avav
        dx, dy, cn = p["dx"], p["dy"], p["cn"]
        gx, gy = cn[None, :, 0] * dx + cn[None, :, 1] * dy, cn[None, :, 1] * dx + cn[None, :, 2] * dy
        terms = {("v_opacity", 0): (vav, 1.0), ("v_conic", 0): (dt(0.5) * vs * dx * dx, 0.5 * dx * dx), ("v_conic", 1): (vs * dx * dy, dx * dy),
                 ("v_conic", 2): (dt(0.5) * vs * dy * dy, 0.5 * dy * dy), ("v_xy", 0): (vs * gx, gx), ("v_xy", 1): (vs * gy, gy)}
        for (key, c), (gr, geo) in terms.items():
            S[key][gid, c] += cs._psum(gr, dt)
            A[key][gid, c] += ((Avav if key == "v_opacity" else Avs) * np.abs(np.asarray(geo, F64))).sum(0)
    return {k: (S[k].astype(F64), A[k]) for k in KEYS}


def reference(sc, cset, mode, dt=F64, fault=None):
    """pair_backward of a scene under a cotangent set, cached"""
    key = ("ref", sc["name"], sc["view"], id(sc), cset, mode, dt, fault)
    if key not in _CACHE:
        _CACHE[key] = pair_backward(sc, cotangent(sc, cset), mode, dt, fault)
    return _CACHE[key]


def row_errors(got, ref):
    """{key: worst row error} of got = {key: array or (array, _)} against a reference(...) result"""
    out = {}
    for k in KEYS:
        g = got[k][0] if isinstance(got[k], tuple) else got[k]
        out[k] = cs.row_errors(np.asarray(g, F64).reshape(ref[k][0].shape), ref[k][0], ref[k][1])[0]
    return out


def reference_distances():
    """worst row error of the float32 closed form against the float64 one per output over every scene, depth map and cotangent set: what
    BARS is eight times of"""
    if "dist" not in _CACHE:
        worst = dict.fromkeys(KEYS, 0.0)
        for name in cs.SCENES:
            sc = cs.scene(name)
            for mode in MODES:
                for cset in CSETS:
                    for k, e in row_errors(reference(sc, cset, mode, F32), reference(sc, cset, mode, F64)).items():
                        worst[k] = max(worst[k], e)
        _CACHE["dist"] = worst
    return _CACHE["dist"]


def forward_distances():
    if "fdist" not in _CACHE:
        worst = dict.fromkeys(FWD_BARS, 0.0)
        for name in cs.SCENES:
            sc = cs.scene(name)
            for mode in MODES:
                for k, e in forward_errors(forward(sc, mode, F32), forward(sc, mode, F64)).items():
                    worst[k] = max(worst[k], e)
        _CACHE["fdist"] = worst
    return _CACHE["fdist"]


def mutant_factors(fault):
    """{(scene, mode): worst over the outputs and cotangent sets of (row error of the float64 mutant against the reference) / bar}"""
    out = {}
    for name in cs.SCENES:
        sc = cs.scene(name)
        for mode in MODES:
            worst = 0.0
            for cset in CSETS:
                for k, e in row_errors(reference(sc, cset, mode, F64, fault), reference(sc, cset, mode, F64)).items():
                    worst = max(worst, e / BARS[k])
            out[(name, mode)] = worst
    return out
