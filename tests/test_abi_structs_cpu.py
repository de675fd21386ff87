"""One definition of the C ABI, include/mmego_hip.h, read by three parties:
  * mmego_amd/hip.py builds its ctypes.Structure classes and argtypes from the header's text.  Here the header is compiled with gcc (it is
    plain C) into a program that prints sizeof and every field's offset; the classes the reader made must agree field by field.
  * every kernel file includes the header through csrc/common.h, so a definition that differs from its declaration does not compile, and the
    launchers read the header's descriptor types (lstm.hip's by-value kernel parameter structs are held to them by a static_assert over
    every field).  Here: a wrong definition is rejected by the compiler.
  * mmego_amd/build.py counts the header among every object's dependencies."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmego_hip.h")


def _c_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        # "const float* a", "int B, T", "const float* xproj[2]", "MmegoBnRef bn1": the first declarator is the last word of the first
        # comma segment, the others are the remaining segments
        segs = decl.split(",")
        for d in [segs[0].replace("*", " ").split()[-1]] + segs[1:]:
            fields.append(re.sub(r"[\*\s]|\[.*\]", "", d))
    return fields


def test_every_descriptor_struct_matches_its_ctypes_mirror(tmp_path):
    from mmego_amd import hip
    text = open(HEADER).read()
    declared = set(re.findall(r"typedef struct (\w+) \{", text))
    PAIRS = {cname: cname[len("Mmego"):] for cname in declared}             # (the name rule of hip.parse_structs)
    assert len(declared) == 8 and declared == set(hip.parse_structs(hip.header_text())), "a struct of the header has no class in hip.py"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HEADER, "int main(void) {"]
    for cname in PAIRS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in _c_fields(text, cname):
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        got.setdefault(s, {})[f] = int(v)
    for cname, pyname in PAIRS.items():
        cls = getattr(hip, pyname)
        assert ctypes.sizeof(cls) == got[cname]["sizeof"], (cname, ctypes.sizeof(cls), got[cname]["sizeof"])
        py = {n: getattr(cls, n).offset for n, _ in cls._fields_}
        c = {k: v for k, v in got[cname].items() if k != "sizeof"}
        assert list(py) == list(c), (cname, "field names / order", list(py), list(c))
        assert py == c, (cname, py, c)


def test_the_struct_reader_refuses_what_it_does_not_know():
    from mmego_amd import hip
    ok = hip.parse_structs("typedef struct MmegoT { const float* a[2]; long b, c; unsigned d; } MmegoT;")["MmegoT"]
    assert ok.__name__ == "T" and [n for n, _ in ok._fields_] == ["a", "b", "c", "d"] and ctypes.sizeof(ok) == 40
    for body in ("short a;", "int a : 3;", "int (*f)(int);", "float* a, *b;", "MmegoLater x;", "int a[N];"):
        with pytest.raises(RuntimeError, match="mmego_hip.h"):
            hip.parse_structs("typedef struct MmegoT { %s } MmegoT;" % body)
    with pytest.raises(RuntimeError, match="mmego_hip.h"):
        hip.parse_structs("typedef struct Other { int a; } Other;")
    with pytest.raises(RuntimeError, match="mmego_hip.h"):
        hip.parse_protos("int mmego_x(void* stream, short n);")


DEFINITIONS = {
    "mmego_fill": ("void* stream, float* X, long n, float v", "void* stream, float* X, int n, float v"),
    "mmego_pack_multi": ("void* stream, int n, const MmegoPack* descs", "void* stream, int n, const MmegoSlab* descs"),
}


@pytest.mark.parametrize("name", sorted(DEFINITIONS))
def test_a_definition_that_differs_from_its_declaration_does_not_compile(tmp_path, name):
    """A kernel file -- anything that includes csrc/common.h -- whose definition of an entry point has another parameter list than the
    header's declaration is rejected ("conflicting types"); the same file with the declared types passes.  Host pass only, no code made."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    runs = []
    for kind, params in zip(("right", "wrong"), DEFINITIONS[name]):
        src = tmp_path / ("%s.hip" % kind)
        src.write_text('#include "%s"\nextern "C" int %s(%s) { return 0; }\n' % (os.path.join(ROOT, "mmego_amd", "csrc", "common.h"), name, params))
        runs.append(subprocess.Popen([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-fsyntax-only", str(src)], stderr=subprocess.PIPE,
                                     text=True))
    (right_err, wrong_err), (right, wrong) = [r.communicate()[1] for r in runs], runs
    assert right.returncode == 0, right_err
    assert wrong.returncode != 0 and "conflicting types for '%s'" % name in wrong_err, wrong_err


def test_the_header_is_a_build_dependency(monkeypatch):
    """With only the header newer than the library and the objects, the library is stale and no object is kept (the freshness predicate
    both build.stale() and compile_one use; nothing is built here)."""
    from mmego_amd import build, hip
    assert os.path.samefile(build.HEADER, hip.HEADER) and build.HEADER in build.shared_deps()
    deps = build.shared_deps()
    assert os.path.abspath(build.__file__) in deps and all(os.path.join(build.CSRC, f) in deps for f in os.listdir(build.CSRC) if f.endswith(".h"))
    src = build.sources()[0]
    obj = os.path.join(build.HERE, "build", os.path.basename(src)[:-4] + ".o")
    newer = set()
    monkeypatch.setattr(os.path, "exists", lambda p: True)
    monkeypatch.setattr(os.path, "getmtime", lambda p: 300.0 if p in newer else 200.0 if p in (build.LIB, obj) else 100.0)
    assert not build.stale() and build.fresh(obj, [src] + build.shared_deps())
    newer.add(build.HEADER)
    assert build.stale() and not build.fresh(obj, [src] + build.shared_deps())
    newer.clear()
    newer.add(src)
    assert build.stale() and not build.fresh(obj, [src] + build.shared_deps())


def test_mmego_gemm_parameters_are_the_gemm_descriptor_fields(monkeypatch):
    """gemm_group fills an MmegoGemmDesc from a recorded mmego_gemm argument list by NAME order: the two orders are checked once by
    hip.lib(), before anything is loaded.  A header in which two long parameters of mmego_gemm are swapped is refused."""
    from mmego_amd import hip
    text = hip.header_text()
    hip.check_gemm_desc(hip.parse_protos(text), hip.parse_structs(text)["MmegoGemmDesc"])
    assert [n for _, n in hip.parse_protos(text)["mmego_gemm"]] == ["stream"] + [n for n, _ in hip.GemmDesc._fields_]
    assert text.count("long sam, long sak") == 1
    swapped = hip.parse_protos(text.replace("long sam, long sak", "long sak, long sam"))
    assert [t for t, _ in swapped["mmego_gemm"]] == [t for t, _ in hip.parse_protos(text)["mmego_gemm"]]      # (types alone cannot tell)
    monkeypatch.setattr(hip, "_protos", swapped)
    monkeypatch.setattr(hip, "_lib", None)
    with pytest.raises(RuntimeError, match="mmego_gemm's parameters"):
        hip.lib()
