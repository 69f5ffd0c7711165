"""CPU: the distortion map (include/ext/gaussctrl_distort.h) as far as it goes without a GPU.  The float64 closed form of tests/_distort_ref.py
against central differences and against the pairwise form, its bars against the float32 mirror they come from, the mutants the bars must
catch; the header against the second table of gaussctrl_amd/_lib.py, the export and typing of the two entry points, their argument checks
(GC_EINVAL before anything is launched: the dummy host buffers are never touched) and the pinned views of the first table; the
private-memory metadata of the two kernels; the model's config fields."""
import ctypes
import os
import re

import numpy as np
import pytest

import _abi_header as A
import _composite_scene as cs
import _distort_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "ext/gaussctrl_distort.h"
NAMES = ["gcx_distort_fwd_views", "gcx_distort_bwd_views"]
EINVAL = -1
F64 = np.float64


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    return os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")


# ---------------------------------------------------------------------------------------- the closed form
def _pixels(sc, tl, q, n=5):
    """a handful of pixel rows of tile tl: the ones with the most, the fewest (but >= 2) and a median number of replayed entries, a stopped
    one and one that owns a capped pair, where the tile has them"""
    cnt = q["con"].sum(1)
    rows = np.nonzero(cnt >= 2)[0]
    if not len(rows):
        return []
    order = rows[np.argsort(cnt[rows], kind="stable")]
    pick = {int(order[0]), int(order[-1]), int(order[len(order) // 2])}
    stopped = rows[q["p"]["stopped"][rows]]
    capped = rows[(q["con"] & (q["p"]["araw"] > F64(cs.ALPHA_CAP)))[rows].any(1)]
    for extra in (stopped, capped):
        if len(extra):
            pick.add(int(extra[0]))
    return sorted(pick)[:n]


@pytest.mark.parametrize("mode", dr.MODES)
@pytest.mark.parametrize("name", cs.SCENES)
def test_closed_form_agrees_with_central_differences(name, mode):
    """dD/dalpha_i and dD/dt_i of the back-to-front replay against central differences of the definition (pixel_distort, a plain loop over
    the pixel's composited entries), and the forward map against the same loop.  Step 1e-6 in alpha (1 - alpha >= 1e-3) and in t: the
    truncation term is ~1e-12 of the gradient's scale and the rounding term 1e-16 |D| / 1e-6, so 1e-7 of (largest |gradient| + |D|) is
    three orders above both"""
    sc = cs.scene(name)
    fw = dr.forward(sc, mode)
    checked = 0
    for tl in range(len(sc["tile_bins"])):
        q = dr.pair_terms(sc, tl, mode)
        if q is None:
            continue
        p = q["p"]
        for r in _pixels(sc, tl, q):
            con = q["con"][r]
            alpha, t = p["alpha"][r, con].astype(F64), q["t"][con].astype(F64)
            D = dr.pixel_distort(alpha, t)
            den = fw["den_distort"][p["py"][r], p["px"][r]]
            assert abs(fw["distort"][p["py"][r], p["px"][r]] - D) <= 1e-13 * max(den, 1e-300)
            da, dtt = q["da"][r, con], q["dtt"][r, con]
            scale = max(np.abs(da).max(), np.abs(dtt).max()) + abs(D)
            h = 1e-6
            for i in range(len(alpha)):
                for arr, want in ((alpha, da[i]), (t, dtt[i])):
                    hi, lo = arr.copy(), arr.copy()
                    hi[i] += h; lo[i] -= h
                    args = (lambda x: (x, t)) if arr is alpha else (lambda x: (alpha, x))
                    cd = (dr.pixel_distort(*args(hi)) - dr.pixel_distort(*args(lo))) / (2 * h)
                    assert abs(cd - want) <= 1e-7 * scale, (name, mode, tl, r, i, cd, want)
            checked += 1
    assert checked >= (2 if name == "tiny" else 5)


@pytest.mark.parametrize("name", cs.SCENES)
def test_forward_is_the_pairwise_sum_where_t_is_sorted(name):
    """every list of a scene is a prefix of one depth order: with depths that increase along it, the prefix form is
    sum_i sum_j w_i w_j |t_i - t_j| at every pixel, under both depth maps (m is increasing)"""
    sc = cs.scene(name)
    full = max(range(len(sc["tile_bins"])), key=lambda tl: sc["tile_bins"][tl][1] - sc["tile_bins"][tl][0])
    s, e = sc["tile_bins"][full]
    order = sc["ids_sorted"][s:e]
    assert len(set(order.tolist())) == len(order) == sc["N"]
    z = np.empty(sc["N"], np.float32)
    z[order] = np.sort(sc["extra"])
    sorted_sc = dict(sc, extra=z)
    for mode in dr.MODES:
        fw = dr.forward(sorted_sc, mode)
        worst = 0.0
        for tl in range(len(sc["tile_bins"])):
            p = cs.tile_pairs(sorted_sc, tl, F64)
            if p is None:
                continue
            t, _ = dr.mapped(z[p["gid"]], mode, F64)
            assert np.all(np.diff(t) >= 0)
            w = np.where(p["contrib"], p["alpha"] * p["T_excl"], 0.0)
            pair = np.einsum("pi,pj,ij->p", w, w, np.abs(t[:, None] - t[None, :]))
            got, den = fw["distort"][p["py"], p["px"]], fw["den_distort"][p["py"], p["px"]]
            live = den > 0
            assert np.all(got[~live] == 0) and np.all(pair[~live] == 0)
            # A_i = 1 - T_i carries one rounding of 1 (1.1e-16) where the pairwise form sums the weights: 1e-12 of the term-wise sum holds both
            if live.any():
                worst = max(worst, float((np.abs(got - pair)[live] / den[live]).max()))
        assert worst <= 1e-12, (name, mode, worst)


def test_bar_window():
    """the bars are 8 x the float32 mirror's distance, rounded down to two digits: 2 x measured <= bar <= 8 x measured"""
    for bars, measured in ((dr.BARS, dr.reference_distances()), (dr.FWD_BARS, dr.forward_distances())):
        assert set(bars) == set(measured)
        for k, m in measured.items():
            assert m > 0 and 2 * m <= bars[k] <= 8 * m, (k, m, bars[k])


@pytest.mark.parametrize("fault", dr.MUTANTS)
def test_every_mutant_misses_the_bars(fault):
    """each mutant of the float64 closed form misses a bar by a factor of 100 at least on one scene (measured, worst output over bar:
    no_r 4600 to 119000, s_after 8700 to 258000, b_wrong 267000 to 430000 on every scene and map; no_dm 1.4e7 to 1.7e7 under map 1 and
    exactly nothing under map 0; cap_passes 3400 / 547 (map 0 / 1) on `opaque`, the one scene with capped pairs, and exactly nothing
    elsewhere)"""
    f = dr.mutant_factors(fault)
    assert max(f.values()) >= 100, f
    if fault == "no_dm":
        assert all(v == 0 for (_, mode), v in f.items() if mode == 0) and all(v >= 100 for (_, mode), v in f.items() if mode == 1), f
    elif fault == "cap_passes":
        assert all((v >= 100) == (name == "opaque") and (v == 0) == (name != "opaque") for (name, _), v in f.items()), f
    else:
        assert all(v >= 100 for v in f.values()), f


# ---------------------------------------------------------------------------------------- the ABI
def test_second_table_is_the_header(built):
    from gaussctrl_amd import _lib
    assert list(_lib.EXT_ABI) == [HEADER]
    protos = A.prototypes(HEADER)
    assert [p.name for p in protos] == list(_lib.EXT_ABI[HEADER]) == NAMES
    assert sorted(NAMES) == A.names(HEADER, "gcx") and A.names(HEADER, "gc") == []
    for p in protos:
        ret, letters = A.signature(p)
        kind, got = _lib.EXT_ABI[HEADER][p.name].split(":")
        assert got == letters and kind == "e" and ret == "i" and letters.endswith("s") and "s" not in letters[:-1], (p.name, got, letters)
    # the backward takes the forward's inputs, letter by letter, in front of its own
    fwd, bwd = (dict(zip(NAMES, protos))[n].params for n in NAMES)
    assert bwd[:len(fwd) - 3] == fwd[:-3]
    # exported, typed, and callable through the one call path
    raw = ctypes.CDLL(built)
    lib = _lib.lib()
    for n in NAMES:
        assert hasattr(raw, n), n
        kind, letters = _lib.EXT_ABI[HEADER][n].split(":")
        fn = getattr(lib, n)
        assert list(fn.argtypes) == [_lib.ARG_TYPES[c] for c in letters] and fn.restype is ctypes.c_int, n
        assert _lib._PLANS[n] == _lib._plan(_lib.EXT_ABI[HEADER][n])
    with pytest.raises(TypeError, match="gcx_distort_fwd_views takes 19 arguments and the stream"):
        _lib.call("gcx_distort_fwd_views", 1, 2, 3)


def test_pinned_views_of_the_first_table_keep_their_sizes():
    from gaussctrl_amd import _lib
    assert len(_lib.SIGNATURES) == 104 and len(_lib.SYMBOLS) == 98 and len(_lib.EXT_SYMBOLS) == 4 and len(_lib.POSE_SYMBOLS) == 2
    assert sorted(_lib.ABI) == A.headers() and set(_lib.EXT_SETS) == {"gaussctrl_bilagrid.h", "gaussctrl_pose.h"}
    assert not set(NAMES) & set(_lib.SIGNATURES)
    assert len(_lib._PLANS) == 106


def test_entry_points_refuse_bad_arguments_before_any_launch(built):
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()                      # host memory: a check that let one of these calls through would not go unnoticed
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    i32, i64, f32 = L.i32, L.i64, L.f32
    nan, inf = float("nan"), float("inf")

    def head(C, N, M, H, W, tx, ty, ptrs, mode, near, far):
        return (i32(C), i64(N), i64(M), i32(1), i32(H), i32(W), i32(tx), i32(ty), *ptrs, i32(mode), f32(near), f32(far))

    def fwd(C=1, N=4, M=8, H=16, W=16, tx=1, ty=1, mode=0, near=0.2, far=100.0, null_at=None, out=(p, p)):
        ptrs = [null if k == null_at else p for k in range(6)]
        return lib.gcx_distort_fwd_views(*head(C, N, M, H, W, tx, ty, ptrs, mode, near, far), *out, null)

    def bwd(C=1, N=4, M=8, H=16, W=16, tx=1, ty=1, mode=0, near=0.2, far=100.0, null_at=None, rest_null=None):
        ptrs = [null if k == null_at else p for k in range(6)]
        rest = [null if k == rest_null else p for k in range(8)]
        return lib.gcx_distort_bwd_views(*head(C, N, M, H, W, tx, ty, ptrs, mode, near, far), *rest, null)

    for f in (fwd, bwd):
        # what gc_trace_mask_views refuses
        assert f(C=0) == EINVAL and f(C=65536) == EINVAL and f(N=-1) == EINVAL and f(M=-1) == EINVAL
        assert f(tx=2) == EINVAL and f(ty=0) == EINVAL and f(H=0) == EINVAL and f(H=17) == EINVAL
        assert b"tile bounds" in lib.gc_last_error_string()
        # the depth map
        assert f(mode=2) == EINVAL and f(mode=-1) == EINVAL
        assert b"depth_map" in lib.gc_last_error_string()
        for near, far in ((0.0, 100.0), (-1.0, 100.0), (5.0, 5.0), (5.0, 1.0), (nan, 100.0), (0.2, nan), (nan, nan), (0.2, inf)):
            assert f(mode=1, near=near, far=far) == EINVAL, (near, far)
        assert b"near_plane" in lib.gc_last_error_string()
        # any NULL array when N > 0
        for k in range(6):
            assert f(null_at=k) == EINVAL, k
        assert b"null argument" in lib.gc_last_error_string()
    assert fwd(out=(null, p)) == EINVAL and fwd(out=(p, null)) == EINVAL
    for k in range(8):
        assert bwd(rest_null=k) == EINVAL, k
    assert b"gcx_distort_bwd_views" in lib.gc_last_error_string()
    # an empty scene: nothing launched (the forward zeroes the images it is given: none here); linear mode does not read the planes
    assert fwd(N=0, null_at=0, out=(null, null)) == 0 and bwd(N=0, null_at=0, rest_null=4) == 0
    assert fwd(N=0, mode=1, near=nan, out=(null, null)) == EINVAL and bwd(N=0, mode=3) == EINVAL
    assert all(v == 0.0 for v in buf)


def test_kernels_use_no_private_memory(built):
    from test_kernel_resources import kernel_resources
    res = kernel_resources(built)
    for name in ("k_distort_fwd", "k_distort_bwd"):
        hit = {k: v for k, v in res.items() if re.search(rf"\b{name}\(", k)}
        assert len(hit) == 1, (name, sorted(hit))
        assert list(hit.values()) == [(0, 0)], hit
    # no counted family of tests/test_kernel_resources.py picks them up
    mine = [k for k in res if "k_distort_" in k]
    assert len(mine) == 2
    for fam in (r"\bk_rasterize_", r"\bk_(refine|mcmc)_", r"\bk_attn", r"\bk_gemm8", r"\bk_thead<", r"\bk_ttail<"):
        assert not [k for k in mine if re.search(fam, k)], fam


# ---------------------------------------------------------------------------------------- the model's switch
def test_config_defaults_and_the_map_name():
    from gaussctrl_amd import gsplat_ops as ops
    from gaussctrl_amd.gc_model import GaussCtrlModelConfig
    cfg = GaussCtrlModelConfig()
    assert cfg.distortion_loss_mult == 0.0 and cfg.distortion_depth_map == "linear"
    assert cfg.distortion_near == 0.2 and cfg.distortion_far == 100.0
    assert GaussCtrlModelConfig(distortion_depth_map="ndc", distortion_loss_mult=0.01).distortion_depth_map == "ndc"
    with pytest.raises(ValueError, match="distortion_depth_map"):
        GaussCtrlModelConfig(distortion_depth_map="disparity")
    aux = ops.RenderAux()
    assert aux.distort is False and aux.distort_depth_map == "linear" and aux.distort_near == 0.2 and aux.distort_far == 100.0
    assert aux.distort_map is None
    with pytest.raises(ValueError, match="distort_depth_map"):
        ops.distort_depth_mode("disparity")
    assert ops.distort_depth_mode("linear") == 0 and ops.distort_depth_mode("ndc") == 1
