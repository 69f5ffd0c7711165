"""Outputs of every attention form, for a bitwise A/B of two builds (the attention kernels have no atomics: a refactor must leave every bit).
    python scripts/attn_forms_dump.py dump OUT.pt [--root DIR]     one fresh process per build; DIR holds the gaussctrl_amd package to load
    python scripts/attn_forms_dump.py compare A.pt B.pt            on the CPU: torch.equal of every kept output, equal digests of the others
Shapes: those of tests/test_attn_forms_gpu.py (heads 2, D 40, 4 frames, bank of 2 x 4: L 256 / 197 with five sets, L 256 with one set, prescaled Q
or not, a spiked key) under every D = 40 form, and one product-shaped launch per kernel (12 frames, 8 heads, the five sets of the cached
reference bank: D 40 / L 4096, D 80 / L 1024, D 160 / L 256 and L 64) under every form that routes it differently.  Outputs up to KEEP bytes
are kept whole; of every output the SHA-256 of its bytes is kept."""
import argparse
import hashlib
import os
import sys

import torch

KEEP = 1 << 20
LOG2E = 1.4426950408889634
FIVE = [(-1, 0.6)] + [(r, 0.1) for r in range(4)]      # = SETS of tests/test_launch_set_kernels_gpu.py: the view itself + its 4 bank references
D40_FORMS = ("0", "RING4", "RING8", "K4", "K4_8WAVE", "K4_Q64", "D40_K3", "ONLINE_ONLY")


def _inputs(dt, f, L, heads, D, seed, pre, spiked=False):
    g = torch.Generator().manual_seed(seed)
    B, C, Lp = 2 * f, heads * D, (L + 7) // 8 * 8
    r = lambda *s: torch.randn(*s, generator=g)
    q, k, v, kr, vr = r(B, L, C), r(B, L, C), r(B, L, C), r(8, L, C), r(8, L, C)
    if spiked:
        k[:, 200] = q[:, 17] * 40.0
    if pre:
        q = q * (D ** -0.5 * LOG2E)

    def t(x):
        out = torch.zeros(x.shape[0], C, Lp)
        out[:, :, :L] = x.transpose(1, 2)
        return out
    return [x.to(dt).to("cuda:0") for x in (q, k, t(v), kr, t(vr))]


def cases():
    """(name, dtype, f, L, heads, D, sets, prescaled, spiked, forms)"""
    for dt in (torch.bfloat16, torch.float16):
        n = str(dt).split(".")[1]
        for L, sets in ((256, FIVE), (197, FIVE), (256, [(-1, 1.0)])):
            for pre in (True, False):
                yield f"{n} small L{L} sets{len(sets)} pre{int(pre)}", dt, 2, L, 2, 40, sets, pre, False, D40_FORMS
        yield f"{n} small L256 sets5 spiked", dt, 2, 256, 2, 40, FIVE, False, True, D40_FORMS
        yield f"{n} product D40 L4096", dt, 6, 4096, 8, 40, FIVE, True, False, D40_FORMS
        yield f"{n} product D80 L1024", dt, 6, 1024, 8, 80, FIVE, True, False, ("0", "ONLINE_ONLY")
        yield f"{n} product D160 L256", dt, 6, 256, 8, 160, FIVE, True, False, ("0", "D160_Q64", "ONLINE_ONLY")
        yield f"{n} product D160 L64", dt, 6, 64, 8, 160, FIVE, True, False, ("0", "ONLINE_ONLY")


def dump(out, root):
    sys.path.insert(0, root)
    from gaussctrl_amd.sd import ops
    assert os.path.abspath(ops.__file__).startswith(os.path.abspath(root)), ops.__file__
    res = {}
    for name, dt, f, L, heads, D, sets, pre, spiked, forms in cases():
        q, k, vt, kr, vtr = _inputs(dt, f, L, heads, D, 1000 + L + D, pre, spiked)
        for form in forms:
            ops.configure(attn_variant=0 if form == "0" else getattr(ops, "GC_ATTN_VAR_" + form))
            log = []
            ops.SELECTION_LOG = log
            o = ops.attention(q, k, vt, heads, sets, f, Lk=L, kref=kr, vtref=vtr, ref_fph=4, q_prescaled=pre).cpu()
            ops.SELECTION_LOG = None
            raw = o.view(torch.int16).numpy().tobytes()
            res[f"{name} {form}"] = {"kernel": log[0][2], "sha256": hashlib.sha256(raw).hexdigest(), "out": o if len(raw) <= KEEP else None}
    ops.configure(attn_variant=0)
    torch.save(res, out)
    print(f"{len(res)} outputs of {os.path.abspath(root)} -> {out}")


def compare(pa, pb):
    a, b = torch.load(pa), torch.load(pb)
    bad = sorted(set(a) ^ set(b))
    for name in sorted(set(a) & set(b)):
        x, y = a[name], b[name]
        same = x["kernel"] == y["kernel"] and x["sha256"] == y["sha256"] and (x["out"] is None or torch.equal(x["out"], y["out"]))
        print(f"{'identical' if same else 'DIFFERENT':9s}  {x['kernel']:13s} {'whole' if x['out'] is not None else 'digest':6s}  {name}")
        if not same:
            bad.append(name)
    print(f"{len(a)} / {len(b)} outputs, {len(bad)} differ or are missing: {'BIT-IDENTICAL' if not bad else bad}")
    return not bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("dump", "compare"))
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    if args.mode == "dump":
        dump(args.paths[0], args.root)
    else:
        sys.exit(0 if compare(*args.paths) else 1)
