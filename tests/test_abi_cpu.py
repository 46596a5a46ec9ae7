"""The C ABI is written down once per side and the two sides agree (no GPU, no build: text).

csrc/kernels/cake_kernels.h (+ driver/graph_loop.h) declares every CAKE_API entry point of the
kernel library; the build proves each definition matches its declaration (a C-linkage
redeclaration with other types does not compile).  What no compiler sees is checked here: the
ctypes table of ops/_lib.py, the constants Python mirrors, and the engine fronts
(engine.py / sd_engine.py against llama_engine.h / sd_engine.h, structs included)."""
import ctypes as C
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "cake_amd" / "csrc"
KERNELS_H = CSRC / "kernels" / "cake_kernels.h"
LOOP_H = CSRC / "driver" / "graph_loop.h"
EXPERIMENTAL_HEADING = "// ==== experimental"

PTR = ("ptr", C.sizeof(C.c_void_p))
VOID = ("void", 0)
C_KINDS = {
    "void": VOID, "float": ("float", 4), "double": ("float", 8),
    "int": ("int", 4), "unsigned": ("int", 4), "unsigned int": ("int", 4),
    "int32_t": ("int", 4), "uint32_t": ("int", 4),
    "long long": ("int", 8), "unsigned long long": ("int", 8),
    "int64_t": ("int", 8), "uint64_t": ("int", 8),
    "size_t": ("int", C.sizeof(C.c_size_t)),
    # handles and callbacks passed by value
    "hipStream_t": PTR, "cake_engine_token_cb": PTR, "cake_token_cb": PTR,
    "cake_announce_cb": PTR,
}
_RET = (r"(?:const\s+)?(?:void|float|double|size_t|u?int(?:32|64)_t|"
        r"(?:unsigned\s+)?(?:long\s+long|int)|unsigned)\s*\**")
PROTO = re.compile(r"(?<![\w.>])(" + _RET + r")\s*\b(cake_\w+)\s*\(([^;{}]*?)\)\s*;")
DEFN = re.compile(r"^CAKE_API\s+[\w\s\*]+?\b(cake_\w+)\s*\(", re.M)


def strip_comments(text: str) -> str:
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def c_kind(decl: str):
    """Kind and width of a C parameter / field / result type (any name already removed)."""
    if "*" in decl:
        return PTR
    t = " ".join(w for w in decl.split() if w not in ("const", "struct"))
    return C_KINDS[t]


def param_kind(decl: str):
    words = decl.replace("*", " * ").split()
    if len(words) > 1 and words[-1] != "*" and " ".join(words) not in C_KINDS and \
            words[-1] not in ("int", "long", "unsigned"):
        words = words[:-1]   # the parameter's name
    return c_kind(" ".join(words))


def prototypes(text: str) -> list:
    """[(name, result kind, [argument kinds])] of every cake_* prototype in C text."""
    out = []
    for ret, name, args in PROTO.findall(strip_comments(text)):
        args = args.strip()
        kinds = [] if args in ("", "void") else [param_kind(a) for a in args.split(",")]
        out.append((name, c_kind(ret), kinds))
    return out


def py_kind(t):
    """Kind and width of a ctypes type, by what it is and its size (ctypes aliases the
    integer classes of one width, so class identity says nothing)."""
    if t is None:
        return VOID
    if issubclass(t, (C._Pointer, C._CFuncPtr)) or t in (C.c_void_p, C.c_char_p):
        return PTR
    code = t._type_
    if code in "fd":
        return ("float", C.sizeof(t))
    assert code in "bBhHiIlLqQ", t
    return ("int", C.sizeof(t))


def check_bindings(decls: dict, bound: dict, what: str) -> None:
    """bound: name -> (restype, argtypes), each against its declaration."""
    for name, (restype, argtypes) in bound.items():
        assert name in decls, f"{what}: {name} is not declared"
        ret, args = decls[name]
        assert py_kind(restype) == ret, f"{what}: {name} result {restype} vs {ret}"
        got = [py_kind(a) for a in argtypes]
        assert len(got) == len(args), f"{what}: {name} takes {len(args)} arguments, not {len(got)}"
        for i, (g, w) in enumerate(zip(got, args)):
            assert g == w, f"{what}: {name} argument {i}: {argtypes[i]} vs {w}"


@pytest.fixture(scope="module")
def header():
    text = KERNELS_H.read_text()
    assert text.count(EXPERIMENTAL_HEADING) == 1
    core, exp = text.split(EXPERIMENTAL_HEADING)
    return {"core": prototypes(core), "exp": prototypes(exp),
            "loop": prototypes(LOOP_H.read_text()), "text": text}


@pytest.fixture(scope="module")
def decls(header):
    return {n: (r, a) for part in ("core", "exp", "loop") for n, r, a in header[part]}


def test_every_entry_point_is_declared_exactly_once(header):
    declared = [n for part in ("core", "exp", "loop") for n, _, _ in header[part]]
    assert len(declared) == len(set(declared)), sorted(n for n in declared if declared.count(n) > 1)
    defined = []
    for d in ("kernels", "driver", "experimental"):
        for f in sorted((CSRC / d).iterdir()):
            defined += DEFN.findall(f.read_text())
    assert len(defined) == len(set(defined))
    assert set(defined) == set(declared), sorted(set(defined) ^ set(declared))
    assert len(defined) > 100   # the scan found the library, not an empty directory
    said = header["text"].split(EXPERIMENTAL_HEADING)[1].split("\n\n")[0]
    assert "only in" in said and "CAKE_BUILD_EXPERIMENTAL=1" in said


def test_one_api_macro_and_no_prototypes_outside_headers():
    hits = [f for f in CSRC.rglob("*") if f.is_file() and "#define CAKE_API" in f.read_text()]
    assert hits == [KERNELS_H]
    for f in CSRC.rglob("*"):
        if f.is_file() and f.suffix != ".h":
            assert not prototypes(f.read_text()), (f, prototypes(f.read_text())[0][0])


def test_python_table_matches_the_header(header, decls):
    from cake_amd.ops import _lib
    check_bindings(decls, _lib._SIGS, "ops/_lib.py")
    assert list(_lib._SIGS) == [n for part in ("core", "loop", "exp") for n, _, _ in header[part]]
    assert _lib._OPTIONAL == {n for n, _, _ in header["exp"]}
    # nothing else in the package binds kernel entry points by hand
    pkg = CSRC.parent
    for f in pkg.rglob("*.py"):
        if f.name not in ("engine.py", "sd_engine.py", "_lib.py"):
            assert not re.search(r"\.(argtypes|restype)\s*=", f.read_text()), f


def test_epilogue_ids_match_the_header(header):
    from cake_amd.ops import gemm, hip
    text = strip_comments(header["text"])
    body = re.search(r"enum GemmEpi : int \{(.*?)\};", text, re.S).group(1)
    ids = {k: int(v) for k, v in re.findall(r"(kEpi\w+)\s*=\s*(\d+)", body)}
    assert len(ids) == 10
    name = lambda key: "kEpi" + "".join(p.capitalize() for p in key.split("_"))  # noqa: E731
    assert {name(k): v for k, v in gemm.EPI.items()}.items() <= ids.items()
    assert set(ids) - {name(k) for k in gemm.EPI} == {"kEpiPartial"}   # kernel-internal
    assert {name(k): v for k, v in hip.W8A8_EPI.items()}.items() <= ids.items()


def c_structs(text: str) -> dict:
    """name -> [(field, kind)] of every struct in C text; int32_t / uint64_t / float /
    double / pointer fields (function pointers included)."""
    out = {}
    for name, body in re.findall(r"struct (Cake\w+) \{(.*?)\n\}", strip_comments(text), re.S):
        fields = []
        for stmt in body.split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            fn = re.match(r".*\(\*\s*(\w+)\)\s*\(", stmt)
            if fn:
                fields.append((fn.group(1), PTR))
                continue
            first, *more = [p.strip() for p in stmt.split(",")]
            m = re.match(r"(.*?[\s\*])(\w+)$", first)
            base, stars = m.group(1).rstrip(), m.group(1).count("*")
            kind = c_kind(base)
            if kind[0] == "int" and base.split()[-1].startswith("u"):
                kind += ("unsigned",)
            fields.append((m.group(2), kind))
            for extra in more:   # `int32_t rank, world;`
                assert "*" not in extra and not stars
                fields.append((extra, kind))
        out[name] = fields
    return out


class _Recorder:
    """Stands in for a loaded library: keeps what a front's _bind sets on each function."""

    class Fn:
        pass

    def __init__(self):
        self.fns = {}

    def __getattr__(self, name):
        return self.fns.setdefault(name, self.Fn())


@pytest.mark.parametrize("mod,hdr", [("cake_amd.engine", "engine/llama_engine.h"),
                                     ("cake_amd.sd_engine", "engine/sd_engine.h"),
                                     ("cake_amd.ops.graph_loop", "driver/graph_loop.h")])
def test_engine_fronts_match_their_headers(mod, hdr):
    import importlib
    m = importlib.import_module(mod)
    text = (CSRC / hdr).read_text()
    if hasattr(m, "_bind"):
        rec = _Recorder()
        m._bind(rec)
        protos = {n: (r, a) for n, r, a in prototypes(text)}
        assert set(rec.fns) == set(protos), sorted(set(rec.fns) ^ set(protos))
        check_bindings(protos, {n: (f.restype, f.argtypes) for n, f in rec.fns.items()}, mod)
    structs = c_structs(text)
    mirrors = {n: t for n, t in vars(m).items() if isinstance(t, type)
               and issubclass(t, C.Structure) and t.__module__ == mod}
    assert mirrors and {"Cake" + n for n in mirrors} <= set(structs)
    if hasattr(m, "_bind"):
        assert {"Cake" + n for n in mirrors} == set(structs)
    for n, t in mirrors.items():
        want = structs["Cake" + n]
        assert [f[0] for f in t._fields_] == [f for f, _ in want], n
        for (fname, ftype), (_, kind) in zip(t._fields_, want):
            got = py_kind(ftype)
            if got[0] == "int" and ftype._type_.isupper():
                got += ("unsigned",)
            assert got == kind, f"{n}.{fname}: {ftype} vs {kind}"
