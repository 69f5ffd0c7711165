"""Per-kernel code comparison of two builds of libgaussctrl_hip.so (a refactor's evidence that the machine code is the parent's).
For every kernel symbol of either library: code size in bytes, a hash of the disassembled instruction text with the addresses (and the
encoding bytes, which hold branch displacements) stripped, and the resource figures of the code object's metadata -- .vgpr_count, .sgpr_count,
.group_segment_fixed_size, .private_segment_fixed_size, .vgpr_spill_count.  It hashes and counts; it looks for no instruction.
    python scripts/kernel_code_diff.py PARENT.so HEAD.so [--filter SUBSTRING] [--all]
prints one row per kernel whose size, hash or figures differ (--all: every kernel), then a summary; exit code 1 when the sets of kernel
symbols differ, a private segment / spill count differs, or a VGPR count / LDS size went up."""
import argparse, hashlib, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from packed_fp32_audit import BIN, code_objects  # noqa: E402

FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")


def kernels(lib):
    """{kernel symbol: dict(size, hash, n_inst, <FIELDS>)} over every gfx950 code object of the library."""
    out = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co); f.flush()
            dis = subprocess.run([f"{BIN}/llvm-objdump", "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([f"{BIN}/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
            syms = subprocess.run([f"{BIN}/llvm-readelf", "-sW", f.name], capture_output=True, text=True, check=True).stdout
        size = {}
        for line in syms.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC":
                size[p[7]] = int(p[2], 0)
        # a kernel's keys are sorted and share one indentation: .group_segment_fixed_size, .name before .private_segment_fixed_size, the rest after
        meta, nl = {}, notes.splitlines()
        for i, line in enumerate(nl):
            m = re.match(r"^(\s+)\.private_segment_fixed_size:\s+(\d+)\s*$", line)
            if not m:
                continue
            ind = re.escape(m.group(1))
            def near(key, lines):
                return next(n.group(1) for n in (re.match(rf"^{ind}\{key}:\s+(\S+)\s*$", l) for l in lines) if n)
            rec = {".private_segment_fixed_size": m.group(2), ".group_segment_fixed_size": near(".group_segment_fixed_size", reversed(nl[:i]))}
            for key in (".sgpr_count", ".vgpr_count", ".vgpr_spill_count"):
                rec[key] = near(key, nl[i:])
            meta[near(".name", reversed(nl[:i])).strip("'\"")] = rec
        name, text = None, {}
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                name = m.group(1); text[name] = []
            elif name and line.strip():
                t = re.sub(r"//.*$", "", line).strip()               # the address comment objdump appends
                t = re.sub(r"<[^>]*>", "<L>", t)                      # branch targets by label, not by address
                if t:
                    text[name].append(t)
        for k, lines in text.items():
            if k not in meta:
                continue                                              # a device function that is no kernel
            shape = [re.sub(r"\b[svak]\d+\b|\b[sva]\[\d+:\d+\]", "R", t) for t in lines]      # the same text with the register numbers blanked
            row = dict(size=size.get(k, 0), n_inst=len(lines), hash=hashlib.sha1("\n".join(lines).encode()).hexdigest()[:12],
                       shape=hashlib.sha1("\n".join(shape).encode()).hexdigest()[:12])
            for fld in FIELDS:
                row[fld] = int(meta[k].get(fld, 0))
            out[k] = row
    return out


def demangle(names):
    d = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent"); ap.add_argument("head")
    ap.add_argument("--filter", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--all", action="store_true", help="print identical kernels too")
    a = ap.parse_args()
    P, H = kernels(a.parent), kernels(a.head)
    names = sorted(set(P) | set(H))
    dm = demangle(names)
    bad = 0
    same = changed = 0
    print(f"# parent {a.parent}\n# head   {a.head}")
    print("# size_p size_h dsize | inst_p inst_h | hash_p hash_h | vgpr p/h | sgpr p/h | lds p/h | private p/h | spill p/h | kernel")
    for k in names:
        if a.filter and a.filter not in dm[k]:
            continue
        p, h = P.get(k), H.get(k)
        if p is None or h is None:
            print(f"{'ONLY IN ' + ('head' if p is None else 'parent'):>20}  {dm[k]}")
            bad += 1
            continue
        ident = p == h
        same += ident; changed += not ident
        if p[".private_segment_fixed_size"] != h[".private_segment_fixed_size"] or p[".vgpr_spill_count"] != h[".vgpr_spill_count"]:
            bad += 1
        if h[".vgpr_count"] > p[".vgpr_count"] or h[".group_segment_fixed_size"] > p[".group_segment_fixed_size"]:
            bad += 1
        if ident and not a.all:
            continue
        print(f"{p['size']:7d} {h['size']:7d} {h['size'] - p['size']:+6d} | {p['n_inst']:6d} {h['n_inst']:6d} | {p['hash']} {h['hash']} "
              f"{'same-shape' if p['shape'] == h['shape'] else 'other-shape'} | "
              + " | ".join(f"{p[f]}/{h[f]}" for f in FIELDS) + f" | {dm[k]}")
    print(f"# {same} kernels identical (size, instruction hash, resources), {changed} differ, {bad} violations "
          "(symbol set, private segment / spills, VGPRs or LDS above the parent's)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
