"""Steady-state loop skeleton of a kernel from hipcc -S --cuda-device-only output: the vmcnt waits, barriers, private-memory (scratch) accesses and
branches of every innermost loop that holds MFMAs and LDS-DMA, with the instructions between them counted by kind.
    python scripts/loop_skeleton.py file.s <mangled kernel symbol>"""
import re, sys
def kernel(path, sym):
    out, on = [], False
    for l in open(path):
        if l.startswith(sym + ":"): on = True
        if on:
            out.append(l.rstrip("\n"))
            if "s_endpgm" in l: break
    return out
def loops(lines):
    """(start, end) of the innermost loops: a label marked 'Inner Loop Header' to the branch back to it"""
    res = []
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):\s+; =>This Inner Loop Header", l)
        if m:
            back = [j for j in range(i + 1, len(lines)) if re.search(r"s_c?branch\w* " + re.escape(m.group(1)) + r"$", lines[j])]
            if back: res.append((i, back[-1]))
    return res
def skeleton(lines, a, b):
    out, n = [], {"v_mfma": 0, "ds_read": 0, "global_load_lds": 0, "salu": 0, "valu": 0}
    def flush():
        s = ", ".join(f"{v} x {k}" for k, v in n.items() if v)
        if s: out.append("        ... " + s)
        for k in n: n[k] = 0
    for l in lines[a:b + 1]:
        t = l.strip()
        if not t or t.startswith(";"): continue
        op = t.split()[0]
        if re.match(r"s_waitcnt|s_barrier|scratch_|s_cbranch|\.LBB", t):
            if op == "s_waitcnt" and "vmcnt" not in t: continue          # lgkmcnt-only waits: LDS reads, not the ring
            flush(); out.append("    " + re.sub(r"\s+", " ", t.split(";")[0]).strip())
        elif op.startswith("v_mfma"): n["v_mfma"] += 1
        elif op.startswith("ds_read"): n["ds_read"] += 1
        elif op.startswith("global_load_lds"): n["global_load_lds"] += 1
        elif op.startswith("s_"): n["salu"] += 1
        elif op.startswith("v_"): n["valu"] += 1
    flush()
    return out
if __name__ == "__main__":
    path, sym = sys.argv[1], sys.argv[2]
    k = kernel(path, sym)
    for a, b in loops(k):
        body = k[a:b + 1]
        if sum("v_mfma" in l for l in body) < 16 or not any("global_load_lds" in l for l in body): continue     # the steady-state loops only
        print(f"  loop at line {a} ({b - a + 1} lines)")
        print("\n".join(skeleton(k, a, b)))
