"""Mechanical checks of the Julia binding (flux3d.jl_amd/julia/Flux3DHip.jl) against the C header.

`julia` is not installed in the build image, so the shim cannot be executed here.  What can be verified
without running it, and is verified on every CPU run:

* every ``@ccall LIB.fx3d_*(arg::Type, ...)::Ret`` against the prototype in include/flux3d_hip.h:
  arity, the C type of every argument, the return type;
* every FX3D_API symbol of the header is bound at least once in the shim (and the ctypes twin agrees
  with the header type by type as well);
* block structure: every ``function`` / ``if`` / ``for`` / ``struct`` / ``module`` / ... has its ``end``,
  brackets balance, no line of code after ``end # module``;
* the interception checklist of INTEGRATION.md section 2a: every reference generic function a
  HipArray-backed TriMesh / PointCloud reaches has a shim method with the expected signature;
* the shim never names CUDA.jl / AMDGPU.jl and is included with a relative ``using ..Flux3D``.
"""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

JL = os.path.join(ROOT, "flux3d.jl_amd", "julia", "Flux3DHip.jl")
HDR = os.path.join(ROOT, "include", "flux3d_hip.h")


# ---------------------------------------------------------------- header side
def _strip_c_comments(txt):
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


HANDLES = {"fx3d_stream_t", "fx3d_event_t", "fx3d_comm_t", "fx3d_graph_t", "fx3d_multi_t"}  # all `void *`


def _norm_ctype(decl):
    """'const float *x' -> ('ptr', 'float');  'int32_t N' -> ('val', 'int32_t');  handles -> ('ptr','void')."""
    decl = decl.strip()
    decl = re.sub(r"\bconst\b", " ", decl)
    stars = decl.count("*")
    decl = decl.replace("*", " ")
    toks = decl.split()
    # drop the parameter name (last token) unless the declaration is a bare type
    base = toks[:-1] if len(toks) > 1 else toks
    base = " ".join(base)
    if base in HANDLES:
        base, stars = "void", stars + 1
    if base == "fx3d_status":
        base = "int32_t"
    if stars == 0:
        return ("val", base)
    if stars == 1:
        return ("ptr", base)
    return ("ptrptr", base)


def parse_header():
    txt = _strip_c_comments(open(HDR).read())
    protos = {}
    for m in re.finditer(r"FX3D_API\s+([\w\s\*]+?)\b(fx3d_\w+)\s*\(([^)]*)\)\s*;", txt, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        argl = [] if args in ("void", "") else [_norm_ctype(a) for a in args.split(",")]
        protos[name] = (_norm_ctype(ret + " _"), argl)
    return protos


# ---------------------------------------------------------------- Julia side
def _strip_jl_comments(txt):
    out = []
    for line in txt.split("\n"):
        # a '#' outside a string literal starts a comment (the shim has no '#' inside strings)
        in_str, res = False, []
        i = 0
        while i < len(line):
            c = line[i]
            if c == '"' and (i == 0 or line[i - 1] != "\\"):
                in_str = not in_str
            if c == "#" and not in_str:
                break
            res.append(c)
            i += 1
        out.append("".join(res))
    return "\n".join(out)


def _balanced(txt, start):
    """txt[start] == '(' -> index just past the matching ')'."""
    depth, i = 0, start
    while True:
        c = txt[i]
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                return i + 1
        i += 1


def _split_top(s):
    parts, depth, cur = [], 0, []
    for c in s:
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
        if c == "," and depth == 0:
            parts.append("".join(cur))
            cur = []
        else:
            cur.append(c)
    if "".join(cur).strip():
        parts.append("".join(cur))
    return parts


def _arg_type(arg):
    """'expr::Type' -> 'Type' (the LAST top-level '::')."""
    depth, pos = 0, -1
    for i, c in enumerate(arg):
        if c in "([{":
            depth += 1
        elif c in ")]}":
            depth -= 1
        elif c == ":" and depth == 0 and arg[i:i + 2] == "::":
            pos = i
    assert pos >= 0, f"@ccall argument without a type annotation: {arg!r}"
    return arg[pos + 2:].strip()


def parse_ccalls():
    txt = _strip_jl_comments(open(JL).read())
    calls = []
    for m in re.finditer(r"@ccall\s+LIB\.(fx3d_\w+)\s*\(", txt):
        name = m.group(1)
        end = _balanced(txt, m.end() - 1)
        args = [_arg_type(a) for a in _split_top(txt[m.end():end - 1])]
        rm = re.match(r"::\s*([\w{}]+)", txt[end:])
        assert rm, f"@ccall {name}: no return type"
        line = txt.count("\n", 0, m.start()) + 1
        calls.append((name, args, rm.group(1), line))
    return calls


JL_ALIASES = {"Stream": "Ptr{Cvoid}", "Event": "Ptr{Cvoid}"}
JL_VAL = {"Int32": "int32_t", "Int64": "int64_t", "UInt64": "uint64_t", "Csize_t": "size_t",
          "Float32": "float", "Float64": "double", "UInt8": "uint8_t"}


JL_STRUCTS = {"MeshRegC": "fx3d_mesh_reg"}  # Julia isbits struct -> the C struct it mirrors field for field


def test_structs_match_the_header():
    """Every struct the shim passes by reference has the header's fields, in order, with matching types (both sides lay isbits
    fields out by the C rules)."""
    hdr = _strip_c_comments(open(HDR).read())
    jl = _strip_jl_comments(open(JL).read())
    for jname, cname in JL_STRUCTS.items():
        cm = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}\s*" + cname + r"\s*;", hdr, flags=re.S)
        assert cm, cname
        cfields = []
        for decl in cm.group(1).split(";"):
            decl = decl.strip()
            if not decl:
                continue
            first, *rest = [d.strip() for d in decl.split(",")]
            ct = _norm_ctype(first)
            cfields.append(ct)
            for r in rest:  # `const int32_t *rowptr, *colind`, `float target, w_lap`: the base type carries over, the stars are per name
                cfields.append(("ptr" if "*" in r else "val", ct[1]))
        jm = re.search(r"\bstruct\s+" + jname + r"\b(.*?)\bend\b", jl, flags=re.S)
        assert jm, jname
        jfields = re.findall(r"\w+::([\w\{\}]+)", jm.group(1))
        assert len(jfields) == len(cfields), (jname, len(jfields), len(cfields))
        for i, (jt, ct) in enumerate(zip(jfields, cfields)):
            ok = (jt == "Ptr{Cvoid}") if ct[0] == "ptr" else JL_VAL.get(jt) == ct[1]
            assert ok, (jname, i, jt, ct)


def _jl_matches(jt, ct):
    """Is the Julia @ccall annotation `jt` a correct way to pass the C parameter `ct`?"""
    jt = JL_ALIASES.get(jt, jt)
    kind, base = ct
    if kind == "val":
        return JL_VAL.get(jt) == base
    if kind == "ptr":
        if jt == "Ptr{Cvoid}":
            return True  # untyped device / handle pointer
        if jt == "Cstring":
            return base == "char"
        m = re.fullmatch(r"(Ptr|Ref)\{(\w+)\}", jt)
        if not m:
            return False
        inner = m.group(2)
        if inner in JL_STRUCTS:  # a struct passed by reference (its fields are checked by test_structs_match_the_header)
            return JL_STRUCTS[inner] == base
        if inner == "T":  # host array of the method's element type: only for `void *`
            return base == "void"
        if inner == "UInt8":
            return base in ("char", "uint8_t", "void")
        return JL_VAL.get(inner) == base
    if kind == "ptrptr":  # out-parameter receiving a pointer / handle, or a host array of device pointers (one per device)
        m = re.fullmatch(r"(Ref|Ptr)\{(.+)\}", jt)
        return bool(m) and JL_ALIASES.get(m.group(2), m.group(2)) == "Ptr{Cvoid}"
    return False


def test_every_ccall_matches_the_header_prototype():
    protos, calls = parse_header(), parse_ccalls()
    assert len(protos) >= 60 and len(calls) >= 70
    bad = []
    for name, args, ret, line in calls:
        if name not in protos:
            bad.append(f"line {line}: {name} is not declared in the header")
            continue
        cret, cargs = protos[name]
        if len(args) != len(cargs):
            bad.append(f"line {line}: {name} arity {len(args)} != {len(cargs)}")
            continue
        for i, (jt, ct) in enumerate(zip(args, cargs)):
            if not _jl_matches(jt, ct):
                bad.append(f"line {line}: {name} arg {i + 1}: Julia `{jt}` vs C {ct}")
        want = {"int32_t": "Int32", "size_t": "Csize_t"}.get(cret[1]) if cret[0] == "val" else "Cstring"
        if ret != want:
            bad.append(f"line {line}: {name} returns `{ret}`, header says {cret}")
    assert not bad, "\n".join(bad)


def test_every_abi_symbol_is_bound_in_the_shim():
    protos = parse_header()
    bound = {c[0] for c in parse_ccalls()}
    assert set(protos) == bound, sorted(set(protos) ^ bound)


def test_ctypes_twin_matches_the_header_types():
    """The executed binding (flux3d.jl_amd/_lib.py) against the same prototypes, type by type."""
    from flux3d_jl_amd import _lib
    protos = parse_header()
    val = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "float": C.c_float, "double": C.c_double}
    bad = []
    for name, (cret, cargs) in protos.items():
        sig = _lib.SIGNATURES[name]
        if len(sig) != len(cargs):
            bad.append(f"{name}: arity {len(sig)} != {len(cargs)}")
            continue
        for i, (pt, (kind, base)) in enumerate(zip(sig, cargs)):
            if kind == "val":
                ok = pt is val[base]
            elif kind == "ptr":
                ok = pt is C.c_void_p or (pt is C.c_char_p and base == "char") or \
                    (hasattr(pt, "_type_") and base in val and pt._type_ is val[base])
            else:
                ok = hasattr(pt, "_type_") and pt._type_ is C.c_void_p
            if not ok:
                bad.append(f"{name} arg {i + 1}: {pt} vs {(kind, base)}")
    assert not bad, "\n".join(bad)


def test_ctypes_struct_matches_the_header():
    """_lib.MeshRegStruct is fx3d_mesh_reg field for field (names, order, types)."""
    from flux3d_jl_amd import _lib
    hdr = _strip_c_comments(open(HDR).read())
    cm = re.search(r"typedef\s+struct\s+fx3d_mesh_reg\s*\{(.*?)\}\s*fx3d_mesh_reg\s*;", hdr, flags=re.S)
    cfields = []
    for decl in cm.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = [d.strip() for d in decl.split(",")]
        ct = _norm_ctype(first)
        cfields.append((first.replace("*", " ").split()[-1], ct))
        for r in rest:
            cfields.append((r.replace("*", " ").strip(), ("ptr" if "*" in r else "val", ct[1])))
    val = {"int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float}
    got = _lib.MeshRegStruct._fields_
    assert [f[0] for f in got] == [f[0] for f in cfields]
    for (name, pt), (_, (kind, base)) in zip(got, cfields):
        assert (pt is C.c_void_p) if kind == "ptr" else (pt is val[base]), (name, pt, kind, base)
    assert C.sizeof(_lib.MeshRegStruct) == 120


# ---------------------------------------------------------------- structure lint
OPENERS = {"function", "if", "for", "while", "let", "try", "begin", "struct", "module", "do", "quote", "macro"}


RUNTESTS = os.path.join(ROOT, "flux3d.jl_amd", "julia", "runtests.jl")


@pytest.mark.parametrize("path", [JL, RUNTESTS], ids=["Flux3DHip.jl", "runtests.jl"])
def test_block_structure_balances(path):
    txt = _strip_jl_comments(open(path).read())
    txt = re.sub(r'"(?:\\.|[^"\\])*"', '""', txt)  # string literals (may hold $(...) interpolation)
    stack, depth_sq = [], 0
    round_curly = []
    for ln, line in enumerate(txt.split("\n"), 1):
        for tok in re.finditer(r"[A-Za-z_][\w!]*|[\[\](){}]|\S", line):
            t = tok.group(0)
            if t == "[":
                depth_sq += 1
            elif t == "]":
                depth_sq -= 1
                assert depth_sq >= 0, f"line {ln}: unbalanced ]"
            elif t in "({":
                round_curly.append((t, ln))
            elif t in ")}":
                assert round_curly, f"line {ln}: unbalanced {t}"
                o, _ = round_curly.pop()
                assert (o, t) in (("(", ")"), ("{", "}")), f"line {ln}: {o} closed by {t}"
            elif t in OPENERS and depth_sq == 0:
                prev = line[:tok.start()].rstrip()
                if t == "struct" and prev.endswith("mutable"):
                    pass
                if t == "if" and round_curly and round_curly[-1][1] == ln and re.search(r"\bfor\b", prev):
                    continue  # generator filter `(x for x in xs if cond)`
                if t == "for" and round_curly and round_curly[-1][1] == ln and prev and prev[-1] not in "(;":
                    continue  # generator / comprehension inside (...)
                stack.append((t, ln))
            elif t in ("elseif", "else", "catch", "finally"):
                assert stack, f"line {ln}: {t} outside a block"
            elif t == "end" and depth_sq == 0:
                assert stack, f"line {ln}: `end` without an opener"
                stack.pop()
    assert not stack, f"unclosed blocks: {stack}"
    assert not round_curly, f"unclosed brackets: {round_curly}"
    assert depth_sq == 0
    if path == JL:
        tail = open(JL).read().rstrip().split("\n")[-1]
        assert tail.startswith("end") and "module" in tail


def test_runtests_uses_only_what_the_shim_and_the_reference_define():
    """julia/runtests.jl (the day-one validation a maintainer with Julia runs) is unexecuted here: what can be
    checked is that every name it takes from the shim is exported or defined there, that it mirrors the reference's own test
    cases (the files it cites exist in INTEGRATION.md's list), and that it never touches CUDA.jl / AMDGPU.jl."""
    src = _strip_jl_comments(open(RUNTESTS).read())
    shim = open(JL).read()
    used = re.search(r"using \.Flux3DHip:(.*?)\n", src).group(1)
    exported = set(re.findall(r"[\w!]+", re.search(r"^export (.*)$", shim, flags=re.M).group(1)))
    for name in re.findall(r"[\w!]+", used):
        assert name in exported, f"{name} is not exported by the shim"
    for qualified in set(re.findall(r"Flux3DHip\.([\w!]+)", src)) - {"jl"}:   # ("Flux3DHip.jl": the file name in the include)
        assert re.search(r"^(?:function |const )?" + re.escape(qualified) + r"(?![\w!])", shim, flags=re.M), qualified  # (names may end in `!`)
    for banned in ("CUDA", "AMDGPU", "CuArray", "ROCArray"):
        assert banned not in src, banned
    assert "include(joinpath(@__DIR__, \"Flux3DHip.jl\"))" in src
    assert "runtests.jl" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---------------------------------------------------------------- interception checklist
# (reference generic function / operation, reference file:line where a HipArray-backed object reaches it,
#  regex of the shim method that must exist)
CHECKLIST = [
    ("TriMesh(verts::Vector{<:CuArray}, faces)", "src/rep/mesh.jl:107-117",
     r"function TriMesh\(verts::Vector\{<:HipArray\{T,2\}\}, faces::Vector\{<:AbstractArray\{R,2\}\};"),
    ("S{T,2}(undef, 3, n) / S{T,3}(undef, 3, V, N)", "src/rep/mesh.jl:151-152",
     r"function HipArray\{T,N\}\(::UndefInitializer, dims::NTuple\{N,Int\}\) where \{T,N\}"),
    ("S{T,N}(undef, dims...)", "src/rep/mesh.jl:151-152",
     r"HipArray\{T,N\}\(::UndefInitializer, dims::Vararg\{Integer,N\}\) where \{T,N\}"),
    ("functor(::TriMesh) rebuild", "src/rep/mesh.jl:189-190", r"\nhip\(m::TriMesh\) = TriMesh\("),
    ("cpu(m)", "src/rep/mesh.jl:189-190", r"\nunhip\(m::TriMesh\) = TriMesh\("),
    ("convert(fieldtype(TriMesh,:_verts_packed), v) in setproperty!", "src/rep/mesh.jl:208-231",
     r"mutable struct HipArray\{T,N\} <: AbstractArray\{T,N\}"),  # convert(::Type{HipArray}, ::HipArray) is the identity
    ("_list_to_packed -> hcat(list...)", "src/rep/utils.jl:95-101",
     r"\n_list_to_packed\(list::Vector\{<:HipArray\{T,2\}\}\) where \{T<:Number\}"),
    ("hcat", "src/rep/utils.jl:98", r"function Base\.hcat\(list::HipArray\{T,2\}\.\.\.\) where \{T\}"),
    ("_packed_to_padded (similar, fill!, setindex!)", "src/rep/utils.jl:119-139",
     r"function _packed_to_padded\(packed::HipArray\{T,2\}, items_len::AbstractArray\{<:Number,1\}, pad_value::Number\)"),
    ("_packed_to_list (getindex ranges)", "src/rep/utils.jl:141-158",
     r"function _packed_to_list\(packed::HipArray\{T,2\}, items_len::AbstractArray\{<:Number,1\}\)"),
    ("_padded_to_list", "src/rep/utils.jl:183-206",
     r"function _padded_to_list\(padded::HipArray\{T,3\}, items_len::Union\{Nothing,AbstractArray\{<:Number,1\}\}\)"),
    ("_padded_to_packed", "src/rep/utils.jl:160-181", r"function _padded_to_packed\(padded::HipArray\{T,3\},"),
    ("_list_to_padded", "src/rep/utils.jl:58-93", r"function _list_to_padded\(list::Vector\{<:HipArray\{T,2\}\},"),
    ("similar(x, dims...)", "src/rep/utils.jl:129, src/transforms/mesh_func.jl:40",
     r"Base\.similar\(a::HipArray, ::Type\{T\}, dims::Dims\{N\}\) where \{T,N\}"),
    ("reshape(areas, 1, :)", "src/rep/mesh.jl:804",
     r"Base\.reshape\(a::HipArray, dims::Tuple\{Vararg\{Union\{Int,Colon\}\}\}\)"),
    ("reshape(points, size..., 1)", "src/rep/pcloud.jl:34", r"Base\.reshape\(a::HipArray, dims::Dims\)"),
    ("T.(v) / Float32.(points)", "src/rep/mesh.jl:129, src/rep/pcloud.jl:46",
     r"Base\.Broadcast\.broadcasted\(::Type\{T\}, a::HipArray\{T\}\) where \{T\} = a"),
    ("packed[:, i:j]", "src/rep/utils.jl:153", r"function Base\.getindex\(a::HipArray\{T,2\}, ::Colon, r::UnitRange\{Int\}\)"),
    ("padded[:, 1:len, i] / p.points[:, :, i]", "src/rep/utils.jl:202, src/rep/pcloud.jl:64",
     r"function Base\.getindex\(a::HipArray\{T,3\}, ::Colon, r::UnitRange\{Int\}, b::Int\)"),
    ("copy(points) in deepcopy_internal(::PointCloud)", "src/rep/pcloud.jl:60-61", r"function Base\.copy\(a::HipArray\{T,N\}\) where \{T,N\}"),
    ("deepcopy(m) in offset", "src/transforms/mesh_func.jl:436", r"Base\.deepcopy_internal\(a::HipArray, dict::IdDict\)"),
    ("verts_packed += offset_verts_packed", "src/transforms/mesh_func.jl:413",
     r"Base\.:\+\(a::HipArray\{Float32,N\}, b::HipArray\{Float32,N\}\) where \{N\}"),
    ("compute_faces_areas_packed(m; eps)", "src/rep/mesh.jl:765-780",
     r"function compute_faces_areas_packed\(m::TriMesh\{Float32,R,HipArray\}; eps::Number = 1e-6\)"),
    ("compute_faces_areas_padded(m; eps)", "src/rep/mesh.jl:799-808",
     r"function compute_faces_areas_padded\(m::TriMesh\{Float32,R,HipArray\}; eps::Number = 1e-6\)"),
    ("sample_points(m, n; eps)", "src/transforms/mesh_func.jl:21-58",
     r"function sample_points\(m::TriMesh\{Float32,R,HipArray\}, num_samples::Int = 5000; eps::Number = Flux3D\.EPS"),
    ("laplacian_loss(m)", "src/metrics/mesh.jl:9-15", r"function laplacian_loss\(m::TriMesh\{Float32,R,HipArray\}\)"),
    ("edge_loss(m, target)", "src/metrics/mesh.jl:24-32",
     r"function edge_loss\(m::TriMesh\{Float32,R,HipArray\}, target_length::Number = 0\.0\)"),
    ("_nearest_neighbors(x, y)", "src/metrics/pcloud.jl:72-86",
     r"function _nearest_neighbors\(x::HipArray\{Float32,3\}, y::HipArray\{Float32,3\}\)"),
    ("_chamfer_distance(A, B, w1, w2)", "src/metrics/pcloud.jl:39-52",
     r"\n_chamfer_distance\(A::HipArray\{Float32,3\}, B::HipArray\{Float32,3\}, w1::Float32 = 1\.0f0, w2::Float32 = 1\.0f0\)"),
    ("Zygote through _chamfer_distance", "src/metrics/pcloud.jl:45-48",
     r"Zygote\.@adjoint function _chamfer_distance\(A::HipArray\{Float32,3\}"),
    ("size(verts, 2) in _compute_edges_packed / _compute_laplacian_packed", "src/rep/mesh.jl:913,965",
     r"Base\.size\(a::HipArray\) = a\.dims"),
    ("show(io, m)", "src/rep/mesh.jl:192-206", r"Base\.show\(io::IO, a::HipArray\{T,N\}\) where \{T,N\}"),
]


def test_interception_checklist_has_a_shim_method_each():
    src = open(JL).read()
    missing = [f"{what} ({where})" for what, where, pat in CHECKLIST if not re.search(pat, src)]
    assert not missing, "\n".join(missing)


DOC_TOKENS = ["TriMesh(::Vector{<:HipArray{T,2}}", "HipArray{T,N}(undef", "Base.Broadcast.broadcasted", "hip(m::TriMesh)",
              "unhip(m::TriMesh)", "setproperty!", "_list_to_packed", "Base.hcat", "_packed_to_padded", "_packed_to_list",
              "_padded_to_list", "_padded_to_packed", "_list_to_padded", "Base.similar", "reshape(::HipArray",
              "getindex(::HipArray{T,2}", "getindex(::HipArray{T,3}", "Base.copy(::HipArray)", "Base.deepcopy_internal",
              "Base.:+", "compute_faces_areas_packed", "sample_points", "laplacian_loss", "edge_loss",
              "_nearest_neighbors", "_chamfer_distance", "Base.size(::HipArray)", "Base.show", "offset!"]


def test_checklist_is_documented_in_integration_md():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "## 2a." in doc
    sec = doc[doc.index("## 2a."):]
    missing = [t for t in DOC_TOKENS if t not in sec]
    assert not missing, missing
    # every reference file the checklist cites is cited in the section
    files = {where.split(":")[0] for _, where, _ in CHECKLIST}
    assert not [f for f in files if f not in sec]


def test_shim_imports_and_dependencies():
    src = _strip_jl_comments(open(JL).read())
    assert re.search(r"^using \.\.Flux3D$", src, flags=re.M), "must be included inside module Flux3D (relative using)"
    assert not re.search(r"^using Flux3D\b", src, flags=re.M)
    for banned in ("CUDA", "AMDGPU", "CuArray", "ROCArray", "KernelAbstractions"):
        assert banned not in src, banned
    # every function the shim extends is imported by name from the parent module
    imp = re.search(r"import \.\.Flux3D:(.*?)\nusing", src, flags=re.S).group(1)
    imported = set(re.findall(r"[\w!]+", imp))
    for fn in ("_list_to_packed", "_packed_to_padded", "_packed_to_list", "_padded_to_list", "_padded_to_packed",
               "_list_to_padded", "compute_faces_areas_packed", "compute_faces_areas_padded", "sample_points",
               "laplacian_loss", "edge_loss", "_nearest_neighbors", "_chamfer_distance", "TriMesh", "offset!"):
        assert fn in imported, fn
    # a method definition `name(` at top level for a reference function that is NOT imported would silently create
    # a new function instead of extending Flux3D's
    defined = set(re.findall(r"^(?:function\s+)?([a-z_][\w!]*)\(.*HipArray", src, flags=re.M))
    reference_names = {"get_verts_packed", "get_verts_padded", "get_verts_list", "get_faces_packed", "get_faces_padded",
                       "get_edges_packed", "get_laplacian_packed", "chamfer_distance", "offset", "normalize!"}
    assert not (defined & reference_names) - imported


def test_imported_names_exist_in_the_reference():
    """Every name the shim imports from Flux3D is defined in the reference sources (tests/golden/ref_definitions.json: the
    functions and mutable structs under the reference's src/, indexed by tests/golden/make_ref_definitions.py)."""
    import json
    src = _strip_jl_comments(open(JL).read())
    imp = re.search(r"import \.\.Flux3D:(.*?)\nusing", src, flags=re.S).group(1)
    names = re.findall(r"[\w!]+", imp)
    with open(os.path.join(ROOT, "tests", "golden", "ref_definitions.json")) as fh:
        defined = json.load(fh)["definitions"]
    assert names
    for n in names:
        assert n in defined, n
