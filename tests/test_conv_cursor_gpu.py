"""GPU: the k-tile cursor of the fast 3x3 convolutions (k_gemm8 MODE 2 / MODE 4, k_gemm8q MODE 2) on every path it takes, and the smallest
k_thead launch.  The cursor -- (tap, channel slice) of the next k-tile to fetch -- is carried by value through the k loop (SGPRs, no private
memory: tests/test_kernel_resources.py); these cases walk it through every wrap it has:

  Cin = 64            one channel slice: the cursor wraps every k-tile (tap-outer) / every 9 k-tiles (tap-inner)
  Cin = 128, 320      2 and 5 slices, against Cout = 128 (NTW 4) and 320 (NTW 5: both W3 copies of the loop)
  MT 2 | 3 | 4        every wave-tile height of the 8-wave kernel (kernel_variant MT field; the planner gives these small grids to the 4-wave kernel)
  k-sliced            B = 2, 16 x 16, Cin = Cout = 320: 45 k-tiles in 3 slices of 15, so slices start at k-tile 15 and 30 = taps 6 and 3 of the
                      tap-inner order (15 % 9, 30 % 9): mid-tap -- the plan is asserted, so the case cannot silently run unsliced
  tap-outer           all of the above with GC_GEMM_VAR_TAP_OUTER
  MODE 4              nearest-x2 upsample fused: 8 x 8 -> 16 x 16, Cin = 128
  fp8                 conv3x3_fp8 at Cin = 128 and 256 (256: two k-slices), both k orders

Reference: torch's fp32 conv2d of the same 2-byte-rounded inputs; bar: the one test_conv3x3 (tests/test_denoise_kernels_gpu.py) uses for the dtype."""
import pytest
import torch
import torch.nn.functional as F

import test_denoise_kernels_gpu as dk
import test_ttail_gpu as tt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 2, 16, 16
CONVS = [(64, 128), (128, 128), (128, 320), (320, 128), (320, 320)]      # (Cin, Cout) at B x 16 x 16
UPS = [(128, 128), (128, 320)]                                           # at B x 8 x 8 -> 16 x 16

_cache = {}


def _case(dt, cin, cout, ups):
    """inputs and fp32 references of one shape, computed once and shared by every kernel variant (never modified)"""
    key = (dt, cin, cout, ups)
    if key not in _cache:
        from gaussctrl_amd.sd.weights import conv3x3_weight
        h, w_ = (H // 2, W // 2) if ups else (H, W)
        x = dk._rand((B, h, w_, cin), dt, 1.0, 1)
        w = dk._rand((cout, cin, 3, 3), dt, (9 * cin) ** -0.5, 2)
        b = torch.randn(cout, generator=torch.Generator().manual_seed(3))
        rv = torch.randn(B, cout, generator=torch.Generator().manual_seed(4))
        res = dk._rand((B, H, W, cout), dt, 1.0, 5)
        xin = x.float().cpu().permute(0, 3, 1, 2)
        if ups:
            xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
        ref = F.conv2d(xin, w.float().cpu(), b, stride=1, padding=1).permute(0, 2, 3, 1)
        ref2 = ref + rv[:, None, None, :] + res.float().cpu()
        _cache[key] = (x, conv3x3_weight(w, dt), b.to(DEV), rv.to(DEV), res, ref, ref2)
    return _cache[key]


@pytest.fixture
def variant(monkeypatch):
    """set gc_gemm_desc.kernel_variant for the test and log what every launch selects"""
    from gaussctrl_amd.sd import ops
    keep = ops.OPTIONS
    log = []
    monkeypatch.setattr(ops, "SELECTION_LOG", log)

    def use(bits):
        ops.configure(gemm_variant=bits)
        del log[:]
        return log
    yield use
    ops.configure(keep)


def _run(dt, cin, cout, ups, log, kernel, mt=None, splits=1):
    from gaussctrl_amd.sd import ops
    x, wp, b, rv, res, ref, ref2 = _case(dt, cin, cout, ups)
    del log[:]
    dk._close(ops.conv3x3(x, wp, b, upsample=ups), ref, dt)                                   # lean epilogue
    dk._close(ops.conv3x3(x, wp, b, upsample=ups, rowvec=rv, residual=res), ref2, dt)
    dk._close(ops.conv3x3(x, wp, b, upsample=ups, act=1), F.silu(ref), dt)                    # plain epilogue (activation)
    if not ups:
        out, _ = ops.conv3x3(x, wp, b, rowvec=rv, residual=res, chan_parts=True)              # channel-partial epilogue where the plan has one
        dk._close(out, ref2, dt)
    assert log, "no launch was logged"
    for _, m, sel in log:
        assert m == B * H * W and sel["kernel"] == kernel and sel["splits"] == splits and sel["ntw"] == (5 if cout == 320 else 4), sel
        assert mt is None or sel["m_tiles"] == mt, sel


@pytest.mark.parametrize("dt", dk.DTS)
@pytest.mark.parametrize("tap_outer", [False, True])
@pytest.mark.parametrize("mt", [2, 3, 4])
def test_conv_cursor_every_wave_tile_and_k_order(dt, tap_outer, mt, variant):
    from gaussctrl_amd.sd import ops
    log = variant((mt << ops.GC_GEMM_VAR_MT_SHIFT) | (ops.GC_GEMM_VAR_TAP_OUTER if tap_outer else 0))
    for cin, cout in CONVS:
        _run(dt, cin, cout, False, log, "k8", mt)
    for cin, cout in UPS:                       # MODE 4
        _run(dt, cin, cout, True, log, "k8", mt)


@pytest.mark.parametrize("dt", dk.DTS)
@pytest.mark.parametrize("tap_outer", [False, True])
def test_conv_cursor_k_slices_start_mid_tap(dt, tap_outer, variant):
    """the planner's own choice for B = 2, 16 x 16, 320 -> 320: the 8-wave kernel in 3 k-slices of 15 of the 45 k-tiles (kt0 = 0, 15, 30)"""
    from gaussctrl_amd.sd import ops
    log = variant(ops.GC_GEMM_VAR_TAP_OUTER if tap_outer else 0)
    _run(dt, 320, 320, False, log, "k8_sliced", 2, splits=3)
    _run(dt, 320, 128, False, log, "k8_sliced", 2, splits=3)


@pytest.mark.parametrize("dt", dk.DTS)
@pytest.mark.parametrize("tap_outer", [False, True])
@pytest.mark.parametrize("cin,cout", [(128, 128), (256, 320)])
def test_conv_cursor_fp8(dt, tap_outer, cin, cout, variant):
    """k_gemm8q: the operands, the fp64 reference and the bar of test_conv3x3_fp8, at the two smallest channel counts (one / two 128-byte slices per
    tap; Cin = 256 runs in two k-slices)"""
    from gaussctrl_amd.sd import ops
    from gaussctrl_amd.sd.weights import conv3x3_weight_fp8
    log = variant(ops.GC_GEMM_VAR_TAP_OUTER if tap_outer else 0)
    dk.test_conv3x3_fp8(dt, B, H, W, cin, cout, 1)            # with the group statistics of its output: never sliced
    assert log and all(sel["kernel"] == "fp8" and sel["splits"] == 1 for _, _, sel in log), log
    # without them the planner slices Cin = 256 in two: the second slice starts at k-tile 9 (tap-outer: tap 4, second channel slice)
    del log[:]
    g = torch.Generator().manual_seed(1)
    x8 = (torch.randn(B, H, W, cin, generator=g) * 1.5).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    w8, wsc = conv3x3_weight_fp8(torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5)
    b = torch.randn(w8.shape[0], generator=g)
    wr = dk._deq(w8, wsc).reshape(-1, 3, 3, cin)[:cout].permute(0, 3, 1, 2)
    ref = F.conv2d(dk._deq(x8).permute(0, 3, 1, 2), wr, b[:cout].double(), padding=1).permute(0, 2, 3, 1)
    got = ops.conv3x3_fp8(x8.to(DEV), w8.to(DEV), wsc.to(DEV), dt, b.to(DEV))
    dk._close(got[..., :cout], ref, dt)
    assert [sel["splits"] for _, _, sel in log] == [cin // 128] and log[0][2]["kernel"] == "fp8", log


@pytest.mark.parametrize("dt", dk.DTS)
def test_head_smallest_launch(dt):
    """k_thead at its smallest legal size (rows_per_frame = 128, B = 2: two workgroups), against the references and bars of
    tests/test_ttail_gpu.py::test_head_matches_torch_and_the_per_op_path"""
    tt.test_head_matches_torch_and_the_per_op_path(dt, 2, 128)
