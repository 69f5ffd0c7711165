"""GPU: the one device-facing piece of the typed binding (gaussctrl_amd/_lib.py) that no kernel test looks at -- call() appends the raw
handle of the CURRENT stream, looked up at every call (the two-stream denoise schedule depends on it).  gc_adam_step on 8 floats through a
recording proxy at `_lib._lib`: the last argument the library receives is the handle of the stream the call was made on, and the step is
torch.optim.Adam's at the bar tests/test_plugin_gpu.py::test_l1_ssim_loss_and_fused_adam holds the fused Adam step to (1e-6, absolute)."""
import pytest
import torch

from _margins import within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Recording:
    """the loaded library, remembering (name, arguments) of what is called through it"""

    def __init__(self, real):
        self.real, self.seen = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def f(*a):
            self.seen.append((name, a))
            return fn(*a)
        return f


@pytest.mark.parametrize("where", ["side", "default"])
def test_call_appends_the_current_stream(where, monkeypatch):
    from gaussctrl_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    p0, grad = torch.randn(8, generator=g), torch.randn(8, generator=g)
    ref = torch.nn.Parameter(p0.clone().to(DEV)); ref.grad = grad.clone().to(DEV)
    torch.optim.Adam([ref], lr=1e-2, betas=(0.9, 0.999), eps=1e-15).step()
    p, gr = p0.clone().to(DEV), grad.clone().to(DEV)
    m, v = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
    default = torch.cuda.current_stream(DEV)
    stream = torch.cuda.Stream(DEV) if where == "side" else default
    proxy = _Recording(L.lib())
    monkeypatch.setattr(L, "_lib", proxy)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        assert L.call("gc_adam_step", p, gr, m, v, 8, 1e-2, 0.9, 0.999, 1e-15, 1) == 0
    stream.synchronize()
    (name, args), = proxy.seen
    assert name == "gc_adam_step" and len(args) == 11
    assert args[:5] == (p.data_ptr(), gr.data_ptr(), m.data_ptr(), v.data_ptr(), 8)
    assert (args[-1] or 0) == (stream.cuda_stream or 0)
    if where == "side":
        assert stream.cuda_stream != default.cuda_stream and args[-1] != (default.cuda_stream or 0)
    within(f"gc_adam_step through call() on the {where} stream vs torch.optim.Adam", float((p - ref.detach()).abs().max()), 1e-6)
