"""The one reader of include/*.h for the tests: comment stripping, the prototypes of a header (return type and parameter types), the
signature letters gaussctrl_amd/_lib.py's table uses, and the argument counter for call sites in host source.  A plain helper module
like _margins.py; the product never parses a header (tests/test_binding_cpu.py holds its table to what this module reads)."""
import ast
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

Proto = collections.namedtuple("Proto", "name ret params")       # params: [(type text, parameter name)]


def headers():
    return sorted(fn for fn in os.listdir(INCLUDE) if fn.endswith(".h"))


def strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def source(header):
    """text of include/<header> without its comments"""
    return strip_comments(open(os.path.join(INCLUDE, header)).read())


def call_args(text, start):
    """number of top-level arguments of the call whose '(' is at text[start]"""
    depth, n, i, seen = 0, 0, start, False
    while True:
        ch = text[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                return n + 1 if seen else 0
        elif ch == "," and depth == 1:
            n += 1
        elif depth >= 1 and not ch.isspace():
            seen = True
        i += 1


def prototypes(header, prefix=r"gcx?_"):
    """the function prototypes of a header, in its order"""
    out = []
    for m in re.finditer(r"\b((?:const\s+)?[a-z0-9_]+[\s\*]+)(" + prefix + r"[a-z0-9_]+)\s*\(([^()]*)\)\s*;", source(header)):
        ret = " ".join(m.group(1).replace("*", " * ").split())
        params = []
        for p in (m.group(3).split(",") if m.group(3).strip() not in ("", "void") else []):
            pm = re.fullmatch(r"(.*?)(\w+)", " ".join(p.replace("*", " * ").split()))
            params.append((pm.group(1).strip(), pm.group(2)))
        out.append(Proto(m.group(2), ret, params))
    return out


def names(header=None, prefix="gc"):
    """sorted names `<prefix>_...(` of a header's text outside comments (header None: of all headers)"""
    src = "".join(source(h) for h in headers()) if header is None else source(header)
    return sorted(set(re.findall(rf"\b({prefix}_[a-z0-9_]+)\s*\(", src)))


def arities(header):
    """{entry point: number of parameters of its prototype}"""
    return {p.name: len(p.params) for p in prototypes(header)}


_LETTER = {"int": "i", "int64_t": "q", "float": "f", "size_t": "z"}
_RETURN = {"int": "i", "size_t": "z", "const char *": "c", "void": "v"}


def signature(proto):
    """(C return type letter, one letter per parameter) in the alphabet of _lib.ABI: i int, q int64_t, f float, z size_t, p any pointer,
    s the trailing `void *stream`"""
    letters = ""
    for k, (ctype, name) in enumerate(proto.params):
        if ctype.endswith("*"):
            letters += "s" if (ctype, name) == ("void *", "stream") and k == len(proto.params) - 1 else "p"
        else:
            letters += _LETTER[ctype]
    return _RETURN[proto.ret], letters


def _tuple_lengths(func, name):
    """lengths of every tuple a function assigns to `name` (plain, chained or unpacking assignment); None for any other value"""
    found = []
    for node in ast.walk(func):
        if isinstance(node, ast.Assign):
            for target in node.targets:
                if isinstance(target, ast.Name) and target.id == name:
                    found.append(node.value)
                elif isinstance(target, ast.Tuple) and isinstance(node.value, ast.Tuple) and len(target.elts) == len(node.value.elts):
                    found += [v for t, v in zip(target.elts, node.value.elts) if isinstance(t, ast.Name) and t.id == name]
    return [_count(func, v.elts) if isinstance(v, ast.Tuple) else None for v in found]


def _count(func, args):
    """arguments a list of call arguments amounts to: a `*name` counts as the tuple the enclosing function assigns to `name`, which must
    have one length wherever it is assigned"""
    n = 0
    for a in args:
        if isinstance(a, ast.Starred):
            assert isinstance(a.value, ast.Name), f"line {a.lineno}: only *name of a local tuple can be counted"
            lengths = set(_tuple_lengths(func, a.value.id))
            assert len(lengths) == 1 and None not in lengths, f"line {a.lineno}: *{a.value.id} is not one tuple of a fixed length: {lengths}"
            n += lengths.pop()
        else:
            n += 1
    return n


def sites(path, header):
    """{entry point of `header`: [arguments the host module passes at each call("<name>", ...) site, the stream call() appends included]}.
    Asserts on the way that the table of gaussctrl_amd/_lib.py has the header's arity for each of them."""
    from gaussctrl_amd import _lib
    want = arities(header)
    for name, n in want.items():
        kind, n_args, stream, _ = _lib._PLANS[name]
        assert n_args + stream == n == len(_lib.SIGNATURES[name].split(":")[1]), name
    out = {}
    for called, n, _ in host_calls(path):
        for name in called:
            if name in want:
                out.setdefault(name, []).append(n + _lib._PLANS[name][2])
    return out


def host_calls(path):
    """[(entry-point name or tuple of names, arguments passed besides the name, line)] of every `call(<name>, ...)` of a host module.  The
    name is a string literal, or `"a" if cond else "b"` (both names); argument tuples handed on with `*` are counted by their elements."""
    tree = ast.parse(open(os.path.join(ROOT, path)).read())
    out = []
    for func in [n for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]:
        for node in ast.walk(func):
            if isinstance(node, ast.Call) and (getattr(node.func, "attr", None) == "call" or getattr(node.func, "id", None) == "call") and node.args:
                if any(isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n is not func and node in ast.walk(n) for n in ast.walk(func)):
                    continue                                    # (belongs to a nested function: counted there)
                first = node.args[0]
                names = [first.body, first.orelse] if isinstance(first, ast.IfExp) else [first]
                assert all(isinstance(n, ast.Constant) and isinstance(n.value, str) for n in names), f"{path}:{node.lineno}: call() without a literal name"
                assert not node.keywords, f"{path}:{node.lineno}: call() is positional"
                out.append((tuple(n.value for n in names), _count(func, node.args[1:]), node.lineno))
    return out
