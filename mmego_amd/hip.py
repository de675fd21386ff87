"""ctypes binding of libmmego_hip.so (the C ABI declared in include/mmego_hip.h).

The prototypes and the descriptor structs (ctypes.Structure classes) are read from the header itself, so binding and
header cannot drift; the kernel files include the same header, so neither can the definitions.  There is NO
fallback: if the library is missing or a kernel launch fails, a RuntimeError is raised.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "mmego_hip.h")
LIBPATH = os.environ.get("MMEGO_HIP_LIB") or os.path.join(_HERE, "lib", "libmmego_hip.so")    # (MMEGO_HIP_LIB: A/B builds of scripts/)

_CT = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double, "unsigned": ctypes.c_uint,
       "unsigned long long": ctypes.c_ulonglong}


def header_text(path=HEADER):
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def _ctype(typ, structs):
    """ctypes type of a C type as the header spells it: any pointer is an address, a descriptor struct by value is its class."""
    typ = typ.replace("const ", "").strip()
    if "*" in typ:
        return ctypes.c_void_p
    if typ not in _CT and typ not in structs:
        raise RuntimeError("mmego_hip.h: type %r is not one this binding reads" % typ)
    return _CT.get(typ) or structs[typ]


def parse_protos(text):
    """-> {name: [(ctype, argname), ...]} for every `int mmego_*(...)` declaration."""
    protos = {}
    for m in re.finditer(r"\bint\s+(mmego_\w+)\s*\(([^)]*)\)\s*;", text):
        args = []
        for a in m.group(2).split(","):
            a = " ".join(a.split())
            if not a or a == "void":
                continue
            name = re.search(r"(\w+)$", a).group(1)
            args.append((_ctype(a[: -len(name)], ()), name))
        protos[m.group(1)] = args
    return protos


def parse_structs(text):
    """-> {C name: ctypes.Structure class} for every `typedef struct MmegoX { ... } MmegoX;`, the class named X.  A member declaration is
    `type a, b;` with type a scalar, a pointer or a struct defined above, and a declarator a name or `name[N]`; anything else raises."""
    structs = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} (\w+);", text, flags=re.S):
        cname, fields = m.group(1), []
        if m.group(3) != cname or not cname.startswith("Mmego"):
            raise RuntimeError("mmego_hip.h: struct %s is not typedef'd as Mmego<Name> under its own name" % cname)
        for decl in m.group(2).split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            d = re.fullmatch(r"([\w ]+?\** ?)(\w+(?:\[\d+\])?(?:, ?\w+(?:\[\d+\])?)*)", decl)
            if not d:
                raise RuntimeError("mmego_hip.h: %s has a member declaration this binding does not read: %r" % (cname, decl))
            typ = _ctype(d.group(1), structs)
            for name in d.group(2).split(","):
                name, _, dim = name.strip().partition("[")
                fields.append((name, typ * int(dim[:-1]) if dim else typ))
        structs[cname] = type(cname[5:], (ctypes.Structure,), {"_fields_": fields, "__doc__": "%s of include/mmego_hip.h." % cname})
    return structs


def parse_tagged_structs(text):
    """-> {C name: class} for every `struct MmegoX { ... }; typedef struct MmegoX MmegoX;` (the tag declared first, the typedef
    behind it): the same members and the same reader as parse_structs, which is handed the one-statement spelling."""
    found = re.findall(r"(?<!typedef )struct (\w+) \{(.*?)\};\s*typedef struct \1 \1;", text, flags=re.S)
    return parse_structs("\n".join("typedef struct %s {%s} %s;" % (n, body, n) for n, body in found))


def parse_header(path=HEADER):
    return parse_protos(header_text(path))


def check_gemm_desc(protos, desc):
    """mmego_gemm's parameters behind the stream are MmegoGemmDesc's fields, in order: gemm_group fills one from the other."""
    params, fields = [n for _, n in protos["mmego_gemm"][1:]], [n for n, _ in desc._fields_]
    if params != fields:
        raise RuntimeError("mmego_hip.h: mmego_gemm's parameters %s are not MmegoGemmDesc's fields %s" % (params, fields))


_protos = parse_header()
_structs = dict(parse_structs(header_text()), **parse_tagged_structs(header_text()))      # (the second: LrSchedule)
globals().update((c.__name__, c) for c in _structs.values())    # GemmDesc, BnRef, GcnFront, Pack, DwRed, Lstm64Fwd, Lstm64Bwd, Slab
_GEMM_PARAMS = [n for _, n in _protos["mmego_gemm"][1:]]
_lib = None


def lib():
    global _lib
    if _lib is None:
        check_gemm_desc(_protos, GemmDesc)
        if not os.path.exists(LIBPATH):
            raise RuntimeError("libmmego_hip.so is not built (%s). Run `python -m mmego_amd.build` "
                               "(or __graft_entry__.build()); there is no CPU fallback." % LIBPATH)
        _lib = ctypes.CDLL(LIBPATH)
        for name, args in _protos.items():
            fn = getattr(_lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = [t for t, _ in args]
    return _lib


def _conv(v):
    if isinstance(v, torch.Tensor):
        return v.data_ptr()
    if isinstance(v, (ctypes.Array, ctypes.Structure)):   # a host-side descriptor (table): kept alive by whoever holds the argument list
        return ctypes.addressof(v)
    return v


def ptr(t):
    """Device address of a tensor (or None / an integer address) for a descriptor field."""
    if t is None:
        return None
    return t.data_ptr() if isinstance(t, torch.Tensor) else int(t)


def is_bf16_mfma_entry(name):
    """True for the entry points (name without the mmego_ prefix) whose kernels run bf16 MFMAs or belong to their chains: everything
    exported by csrc/split3.hip, bf16.hip and *_bf16.hip (tests/test_host_cpu.py checks that no other file contains a bf16 MFMA and
    that every entry point of those files matches).  What the exclusivity check of plan.unordered_with() calls an aggressor."""
    return name.startswith("split3_") or "bf16" in name


def stream_handle():
    return torch.cuda.current_stream().cuda_stream


def _bnref_of(bn, state, rec=None, nrec=0, rows_per_rec=0):
    """A BatchNorm module whose batch statistics arrive as partial records."""
    return BnRef(rec=ptr(rec), nrec=int(nrec), rows_per_rec=int(rows_per_rec), gamma=ptr(bn.weight), beta=ptr(bn.bias),
                 running_mean=ptr(bn.running_mean), running_var=ptr(bn.running_var), momentum=float(bn.momentum), eps=float(bn.eps),
                 state=ptr(state))


BnRef.of = staticmethod(_bnref_of)


def pair2(a, b):
    """Two device addresses as a descriptor's pointer pair."""
    return (ctypes.c_void_p * 2)(ptr(a), ptr(b))


_gemm_rec = None
_gemm_rec_outs = None


class gemm_group:
    """Context: the mmego_gemm calls made inside are collected and issued as ONE mmego_gemm_group launch at exit; every other
    launch inside the context runs immediately.  Contract (checked):
      * independent products only -- a product recorded here is not executed before the context ends, so nothing inside the
        context may read OR write what a recorded product writes (its C and asum): a pass-through launch, or a later recorded
        product, one of whose pointer arguments -- a tensor (any view) or a raw integer address -- falls inside the byte extent
        of a deferred output raises;
      * the group is issued on the stream that was current at entry: a stream switch inside the context raises at exit;
      * split-K products share ops.scratch: the group entry point runs a group containing one as separate launches in recorded
        order on that one stream (mmego_gemm_group's fallback), which keeps the scratch reuse stream-ordered."""

    def __enter__(self):
        global _gemm_rec, _gemm_rec_outs
        if _gemm_rec is not None:
            raise RuntimeError("gemm_group contexts do not nest")
        _gemm_rec, _gemm_rec_outs = [], []
        self._stream = stream_handle()
        return self

    def __exit__(self, et, ev, tb):
        global _gemm_rec, _gemm_rec_outs
        rec, _gemm_rec, _gemm_rec_outs = _gemm_rec, None, None
        if et is None and rec:
            if stream_handle() != self._stream:
                raise RuntimeError("gemm_group: the current stream changed inside the context; the deferred products would be "
                                   "issued on another stream than the launches around them")
            for i in range(0, len(rec), 10):
                part = rec[i:i + 10]
                arr = (GemmDesc * len(part))()
                for dsc, a in zip(arr, part):
                    for fname, v in zip(_GEMM_PARAMS, a):
                        setattr(dsc, fname, _conv(v))
                call("gemm_group", len(part), arr)          # (the array object, not its address: a recorded call keeps it alive)
        return False


def _launch(name, *args):
    """The one place a kernel is launched: `mmego_<name>` on torch's current stream, tensors passed as device pointers.
    (plan.StepPlan swaps this function for a recorder while it records a step.)"""
    fn = getattr(lib(), "mmego_" + name)
    rc = fn(stream_handle(), *[_conv(a) for a in args])
    if rc != 0:
        raise RuntimeError("mmego_%s failed: %s" % (name, "bad argument" if rc < 0 else "hipError %d" % rc))


def _ptr_of(a):
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    if isinstance(a, int) and a >= (1 << 20):        # a raw device address (sizes, strides and flags are far below any mapping)
        return a
    return None


def _gemm_out_extents(args):
    """Byte ranges [lo, hi) a recorded mmego_gemm writes: C (M x N x nbatch through its strides) and asum (M floats per batch)."""
    out, a = [], dict(zip(_GEMM_PARAMS, args))
    M, N, nb = int(a["M"]), int(a["N"]), max(1, int(a["nbatch"]))
    c = _ptr_of(a["C"])
    if c is not None:
        span = (M - 1) * abs(int(a["scm"])) + (N - 1) * abs(int(a["scn"])) + 1
        for b in range(nb):              # (per batch: the batches of a pair product may lie apart, with other leaves' slots between)
            lo = c + 4 * b * int(a["sCb"])
            out.append((lo, lo + 4 * span))
    s = _ptr_of(a["asum"])
    if s is not None:
        out.append((s, s + 4 * M * nb))
    return out


def call(name, *args):
    """Launch `mmego_<name>` on torch's current stream (inside a gemm_group context: defer the mmego_gemm calls)."""
    if _gemm_rec is not None and name != "gemm_group":
        for a in args:
            p = _ptr_of(a)
            if p is not None and any(lo <= p < hi for lo, hi in _gemm_rec_outs):
                raise RuntimeError("gemm_group: mmego_%s takes the output of a product that is still deferred inside this context "
                                   "(only independent leaves may be grouped)" % name)
        if name == "gemm":
            _gemm_rec_outs.extend(_gemm_out_extents(args))
            _gemm_rec.append(args)
            return
    _launch(name, *args)


def graph_dA_nblk(G):
    return lib().mmego_graph_dA_nblk(G)


def colstats_nblk(rows):
    return lib().mmego_colstats_nblk(rows)
