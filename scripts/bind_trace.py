"""Launch-sequence trace of the host layer, for A/B across a change of the binding: every entry point the library is asked for, in order,
with its scalar arguments.  A proxy at `_lib._lib` sees the calls however the host code spells them (wrapped ctypes values or plain Python
ones): ctypes wrappers are unwrapped with .value, floats are rounded to float32 as the ABI takes them, pointers are reduced to NULL /
PTR, the stream is left out, and entry points that take a descriptor struct are recorded by name only.  Which argument is what comes from
the prototypes of include/*.h (tests/_abi_header.py), not from the binding under test.

Workload: __graft_entry__.smoke(), then one tiny training render (300 Gaussians, 32 x 32, one and two views, forward + backward) under
each RenderAux switch: depth_grad, antialiased, absgrad, pose_grad, grad_into with accumulate, m_cap.

    python scripts/bind_trace.py OUT.txt          # two commits' files must be equal line for line (profiles/bind_trace_*.txt)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

import _abi_header as A
from gaussctrl_amd import _lib as L

PROTOS = {p.name: p for h in A.headers() for p in A.prototypes(h)}


def _plain(v):
    return v.value if isinstance(v, ctypes._SimpleCData) else v


def _render(proto, args):
    if proto.params and "_desc" in proto.params[0][0]:
        return proto.name
    out = []
    for (ctype, pname), v in zip(proto.params, args):
        if (ctype, pname) == ("void *", "stream"):
            continue
        if ctype.endswith("*"):
            v = _plain(v)
            out.append("NULL" if v is None or (isinstance(v, int) and v == 0) else "PTR")
        elif ctype == "float":
            out.append(repr(ctypes.c_float(float(_plain(v))).value))
        else:
            out.append(str(int(_plain(v))))
    return f"{proto.name}({', '.join(out)})" + ("" if len(args) == len(proto.params) else f"  !! {len(args)} arguments for {len(proto.params)} parameters")


class Trace:
    def __init__(self, real):
        self.real, self.lines = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name not in PROTOS or name == "gc_last_error_string":
            return fn

        def f(*a):
            self.lines.append(_render(PROTOS[name], a))
            return fn(*a)
        return f


def renders(trace):
    from gaussctrl_amd import gsplat_ops as ops, synthetic as syn
    from gaussctrl_amd.camera import camera_to_gsplat
    dev = "cuda:0"
    N, W, H = 300, 32, 32
    P = syn.make_gaussians(N, seed=0, scale_mean=0.05)
    cams = [camera_to_gsplat(c2w, 30.0, 30.0, 16.0, 16.0, W, H) for c2w in syn.make_cameras(2, seed=1)]
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    keys = ("means", "scales", "quats", "opacities", "features_dc", "features_rest")

    def into():
        return {k: torch.zeros(P[k].shape, device=dev).reshape(-1) if k == "opacities" else torch.zeros(P[k].shape, device=dev) for k in keys}
    switches = [("plain", {}), ("depth_grad", dict(depth_grad=True)), ("antialiased", dict(antialiased=True)), ("absgrad", dict(absgrad=True)),
                ("pose_grad", dict(pose_grad=True)), ("grad_into+accumulate", dict(grad_into=into, grad_accumulate=True)), ("m_cap", dict(m_cap=4096)),
                ("depth_grad+antialiased+absgrad+pose_grad", dict(depth_grad=True, antialiased=True, absgrad=True, pose_grad=True)),
                ("no tight boxes / pair chain", dict(tight_boxes=False, sorted_boxes=False))]
    for label, kw in switches:
        for views in (1, 2):
            trace.lines.append(f"# render: {label}, {views} view(s)")
            aux = ops.RenderAux()
            for k, v in kw.items():
                setattr(aux, k, v() if callable(v) else v)
            tp = [torch.tensor(P[k], device=dev, requires_grad=True) for k in keys]
            if views == 1:
                rgb, alpha, depth = ops.render_view(*tp, cams[0], bg, True, 3, aux)
            else:
                rgb, alpha, depth = ops.render_views(*tp, cams, bg, True, 3, aux)
            loss = rgb.sum() + 0.5 * alpha.sum() + (0.1 * depth.sum() if aux.depth_grad else 0.0)
            loss.backward()
            torch.cuda.synchronize()


def main(out):
    import __graft_entry__ as ge
    trace = Trace(L.lib())
    L._lib = trace
    try:
        trace.lines.append("# smoke()")
        ge.smoke()
        renders(trace)
    finally:
        L._lib = trace.real
    with open(out, "w") as f:
        f.write("\n".join(trace.lines) + "\n")
    print(f"{len(trace.lines)} lines -> {out}")


if __name__ == "__main__":
    main(sys.argv[1])
