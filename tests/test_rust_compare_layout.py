"""The `compare` module of the Rust binding (bindings/rust/src/lib.rs) against include/mp3rgain_amd_compare.h -- without a Rust
toolchain, with the parsers of tests/test_rust_binding_layout.py: the extern declaration of the file call against its prototype,
every #[repr(C)] struct against the C struct's field names, order and types, its size under C's layout rules against ctypes' of
the same struct, and the constants against the header's."""
import ctypes as C
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_rust_binding_layout as base  # noqa: E402
import test_rust_tempo_layout as tempo  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

HEADER = base.ROOT / "include" / "mp3rgain_amd_compare.h"
STRUCTS = {"RgComparePair": ("rg_compare_pair", _capi.ComparePair), "RgCompareOpts": ("rg_compare_opts", _capi.CompareOpts),
           "RgCompareBlock": ("rg_compare_block", _capi.CompareBlock), "RgCompareResult": ("rg_compare_result", _capi.CompareRecord)}


def _module():
    src = base.rust_source()
    return src[src.index("pub mod compare {"):src.index("pub mod clicks {")]


def _c_type(rust):
    quals, t = [], rust.strip()
    while t.startswith("*"):
        q, t = re.match(r"\*(const|mut)\s+(.*)", t).groups()
        quals.append(q)
    c = STRUCTS[t][0] if t in STRUCTS else (base.SCALARS[t][0] if t in base.SCALARS else base.STRUCTS[t])
    for i, q in enumerate(reversed(quals)):
        c = (("const " if q == "const" else "") + c + " *") if i == 0 else (c + (" const" if q == "const" else "") + " *")
    return base._norm_c_type(c)


def test_the_file_call_matches_the_header(monkeypatch):
    monkeypatch.setattr(base, "HEADERS", [HEADER])
    protos = base.c_prototypes()
    assert set(protos) == {"rg_compare", "rg_compare_arena", "rg_compare_kernel_shape", "rg_compare_rate", "rg_compare_error"}
    block = re.search(r'extern "C" \{(.*?)\n    \}', _module(), flags=re.S).group(1)
    ext = re.findall(r"pub fn (\w+)\((.*?)\)\s*->\s*([^;]+?)\s*;", block, flags=re.S)
    assert [n for n, _, _ in ext] == ["rg_compare"]  # the seams and the measurement hook are the tests' and the tools'
    for name, args, ret in ext:
        c_ret, c_params = protos[name]
        params = [tuple(x.strip() for x in a.split(":", 1)) for a in args.split(",") if a.strip()]
        assert [n for n, _ in params] == [n for n, _ in c_params], name
        for (n, rt), (_, ct) in zip(params, c_params):
            assert _c_type(rt) == ct, f"{name}({n}): Rust {rt} is C `{_c_type(rt)}`, the header says `{ct}`"
        assert _c_type(ret) == c_ret, name


def test_structs_match_the_header_and_the_python_binding(monkeypatch):
    monkeypatch.setattr(tempo, "HEADER", HEADER)
    cs = tempo._c_structs()
    found = re.findall(r"#\[repr\(C\)\]\s*///[^\n]*\s*pub struct (\w+) \{(.*?)\n    \}", _module(), flags=re.S)
    assert {n for n, _ in found} == set(STRUCTS)
    for rname, body in found:
        cname, ctype = STRUCTS[rname]
        fields = [(n, t.strip()) for n, t in re.findall(r"pub\s+(\w+):\s*([^,\n]+),", body)]
        cf = cs[cname]
        assert [n for n, _ in fields] == [n for n, _ in cf] == [n for n, _ in ctype._fields_], rname
        for (n, rt), (_, ct), (_, pt) in zip(fields, cf, ctype._fields_):
            assert base.SCALARS[rt][0] == ct, f"{rname}.{n}: Rust {rt}, C `{ct}`"
            assert base.SCALARS[rt][1] == C.sizeof(pt), f"{rname}.{n}"
        # every field is naturally aligned with no padding between them, so #[repr(C)] and C agree when the sizes add up
        assert sum(C.sizeof(pt) for _, pt in ctype._fields_) == C.sizeof(ctype), rname
    assert [C.sizeof(t) for _, t in STRUCTS.values()] == [16, 36, 48, 280]


def test_constants_equal_the_headers():
    hdr = HEADER.read_text()
    c_vals = {n: int(v, 0) for n, v in re.findall(r"#define\s+RG_(CMP_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", hdr)}
    c_vals.update({n: 1 << int(k) for n, k in re.findall(r"#define\s+RG_(CMP_\w+)\s+\(1u << (\d+)\)", hdr)})
    rust = {n: int(v.replace("_", ""), 0) for n, v in re.findall(r"pub const (CMP_\w+):\s*(?:u32|usize)\s*=\s*(0x[0-9A-Fa-f_]+|\d+);", _module())}
    assert len(rust) == 31 and set(rust) == set(c_vals)
    for n, v in rust.items():
        assert c_vals[n] == v, n
        assert getattr(_capi, n) == v, n
    body = re.search(r"impl Default for RgCompareOpts \{(.*?)\n    \}", _module(), flags=re.S).group(1)
    assert re.findall(r"(\w+): (\w+),", body) == [("align", "CMP_ALIGN_FINGERPRINT"), ("coarse_radius", "CMP_DEFAULT_COARSE_RADIUS"), ("radius", "CMP_DEFAULT_RADIUS"),
                                                  ("segments", "CMP_DEFAULT_SEGMENTS"), ("segment_frames", "CMP_DEFAULT_SEGMENT_FRAMES"), ("block_frames", "0"),
                                                  ("drift_frames", "CMP_DEFAULT_DRIFT_FRAMES"), ("lock_permille", "CMP_DEFAULT_LOCK_PERMILLE"),
                                                  ("requant_millilsb2", "CMP_DEFAULT_REQUANT_MILLILSB2")]
