"""CPU: the camera-gradient extension set of the C ABI (include/gaussctrl_pose.h) as far as it goes without a GPU: the header's two gcx_
names, their export and the loader's POSE_SYMBOLS beside unchanged SYMBOLS / EXT_SYMBOLS; the workspace query; the argument checks
(GC_EINVAL before anything is launched: the dummy host buffers are never touched); the private-memory metadata of the new kernels."""
import ctypes
import os
import re

import pytest

from _abi_header import names as _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gcx_pose_bwd_views", "gcx_pose_bwd_views_workspace_bytes"]
EINVAL = -1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")):
        ge.build()
    return os.path.join(ROOT, "gaussctrl_amd", "libgaussctrl_hip.so")


def test_header_declares_the_two_extension_entry_points(built):
    from gaussctrl_amd import _lib
    assert _declared("gaussctrl_pose.h", "gcx") == NAMES
    assert _declared("gaussctrl_pose.h", "gc") == []                      # nothing the counted set's regex would pick up ...
    assert not re.search(r"\bgc_[a-z0-9_]+\s*\(", open(os.path.join(ROOT, "include", "gaussctrl_pose.h")).read())     # ... comments included
    assert sorted(_lib.POSE_SYMBOLS) == NAMES and _lib.EXT_SETS["gaussctrl_pose.h"] is _lib.POSE_SYMBOLS
    assert not set(_lib.POSE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.EXT_SYMBOLS))
    assert len(_lib.SYMBOLS) == len(set(_lib.SYMBOLS)) == 98 and len(_lib.EXT_SYMBOLS) == 4        # the counted set and the grid's set stay
    for header, names in _lib.EXT_SETS.items():                             # every extension header against its list
        assert _declared(header, "gcx") == sorted(names), header
    lib = ctypes.CDLL(built)
    for n in NAMES:
        assert hasattr(lib, n), n
    l = _lib.lib()
    assert l.gcx_pose_bwd_views_workspace_bytes.restype is ctypes.c_size_t and l.gcx_pose_bwd_views.restype is ctypes.c_int


def test_workspace_query(built):
    """one float32 partial [24] per view and workgroup of 1024 Gaussians"""
    from gaussctrl_amd import _lib as L
    q = lambda n, c: L.lib().gcx_pose_bwd_views_workspace_bytes(L.i64(n), L.i32(c))
    assert q(0, 1) == 0 and q(-1, 1) == 0 and q(5, 0) == 0
    assert q(1, 1) == 96 and q(1024, 1) == 96 and q(1025, 1) == 192 and q(299, 9) == 9 * 96
    assert q(1_000_000, 8) == 8 * 977 * 96


def test_entry_point_refuses_bad_arguments_before_any_launch(built):
    from gaussctrl_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()                      # host memory: a check that let one of these calls through would not go unnoticed
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    cams = (ctypes.c_float * 70)()

    def call(N=5, C=2, aa=0, means=p, ls=p, quats=p, op=p, cams=cams, H=8, W=8, radii=p, conics=p, v_xy=p, v_conic=p, v_opac=p, v_depths=p,
             ws=p, out=p):
        return lib.gcx_pose_bwd_views(L.i64(N), L.i32(C), L.i32(aa), means, ls, quats, op, cams, L.i32(H), L.i32(W), radii, conics, v_xy,
                                      v_conic, v_opac, v_depths, ws, out, null)

    assert call(C=0) == EINVAL and call(C=-1) == EINVAL and call(N=-1) == EINVAL and call(cams=null) == EINVAL
    assert b"gcx_pose_bwd_views" in lib.gc_last_error_string()
    assert call(N=(1 << 31) // 6 + 1) == EINVAL and call(N=1 << 40, C=1) == EINVAL          # C * N * 3 >= 2^31
    assert b"2^31" in lib.gc_last_error_string()
    assert call(H=0) == EINVAL and call(W=0) == EINVAL and call(out=null) == EINVAL and call(N=0, out=null) == EINVAL
    for name in ("means", "ls", "quats", "op", "radii", "conics", "v_xy", "v_conic", "ws"):
        assert call(**{name: null}) == EINVAL, name
    assert call(aa=1, v_opac=null) == EINVAL
    assert b"v_opac" in lib.gc_last_error_string()
    assert all(v == 0.0 for v in buf)


def test_new_kernels_use_no_private_memory(built):
    from test_kernel_resources import kernel_resources
    res = kernel_resources(built)
    hit = {k: v for k, v in res.items() if re.search(r"\bk_pose_", k)}
    for name in (r"k_pose_bwd_views<true>", r"k_pose_bwd_views<false>", r"k_pose_sum\("):
        assert sum(bool(re.search(rf"\b{name}", k)) for k in hit) == 1, (name, sorted(hit))
    assert len(hit) == 3, sorted(hit)
    assert all(v == (0, 0) for v in hit.values()), hit
    # the counted families of tests/test_kernel_resources.py and test_bilagrid_abi_cpu.py do not pick them up
    assert not any(re.search(r"\bk_(refine|mcmc|bilagrid)_|\bk_rasterize_|\bk_gemm8|\bk_thead<|\bk_ttail<|\bk_attn5<", k) for k in hit)
