"""The `flacenc` module of the Rust binding (bindings/rust/src/lib.rs) against include/mp3rgain_amd_flacenc.h -- without a Rust
toolchain, with the parsers of tests/test_rust_binding_layout.py: the extern declaration of the file call against its prototype,
every #[repr(C)] struct against the C struct's field names, order and types, its size under C's layout rules against ctypes' of
the same struct, and the constants against the header's."""
import ctypes as C
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_rust_binding_layout as base  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

HEADER = base.ROOT / "include" / "mp3rgain_amd_flacenc.h"
STRUCTS = {"RgFlacEncodeOptions": ("rg_flac_encode_options", _capi.FlacEncodeOptions), "RgFlacEncodeResult": ("rg_flac_encode_result", _capi.FlacEncodeRecord)}


def _module():
    src = base.rust_source()
    return src[src.index("pub mod flacenc {"):src.index("pub mod stereo {")]


def _c_type(rust):
    quals, t = [], rust.strip()
    while t.startswith("*"):
        q, t = re.match(r"\*(const|mut)\s+(.*)", t).groups()
        quals.append(q)
    c = STRUCTS[t][0] if t in STRUCTS else (base.SCALARS[t][0] if t in base.SCALARS else base.STRUCTS[t])
    for i, q in enumerate(reversed(quals)):
        c = (("const " if q == "const" else "") + c + " *") if i == 0 else (c + (" const" if q == "const" else "") + " *")
    return base._norm_c_type(c)


def _c_structs():
    """name -> [(field, C type, array length or None)]; `a, b` declarations are taken apart."""
    out = {}
    src = base._strip_c(HEADER.read_text())
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", src, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ctype, names = decl.split(" ", 1)
            for n in names.split(","):
                m = re.match(r"(\w+)(?:\[(\d+)\])?$", n.strip())
                fields.append((m.group(1), ctype, int(m.group(2)) if m.group(2) else None))
        out[name] = fields
    return out


def test_the_file_call_matches_the_header(monkeypatch):
    monkeypatch.setattr(base, "HEADERS", [HEADER])
    protos = base.c_prototypes()
    assert set(protos) == {"rg_flac_encode_files", "rg_flac_encode_arena", "rg_flac_encode_source_blocks", "rg_flac_encode_rate"}
    block = re.search(r'extern "C" \{(.*?)\n    \}', _module(), flags=re.S).group(1)
    ext = re.findall(r"pub fn (\w+)\((.*?)\)\s*->\s*([^;]+?)\s*;", block, flags=re.S)
    assert [n for n, _, _ in ext] == ["rg_flac_encode_files"]  # the seam and the measurement hook are the tests' and the tools'
    for name, args, ret in ext:
        c_ret, c_params = protos[name]
        params = [tuple(x.strip() for x in a.split(":", 1)) for a in args.split(",") if a.strip()]
        assert [n for n, _ in params] == [n for n, _ in c_params], name
        for (n, rt), (_, ct) in zip(params, c_params):
            assert _c_type(rt) == ct, f"{name}({n}): Rust {rt} is C `{_c_type(rt)}`, the header says `{ct}`"
        assert _c_type(ret) == c_ret, name


def test_structs_match_the_header_and_the_python_binding():
    cs = _c_structs()
    found = re.findall(r"#\[repr\(C\)\]\s*///[^\n]*\s*pub struct (\w+) \{(.*?)\n    \}", _module(), flags=re.S)
    assert {n for n, _ in found} == set(STRUCTS)
    for rname, body in found:
        cname, ctype = STRUCTS[rname]
        fields = [(n, t.strip()) for n, t in re.findall(r"pub\s+(\w+):\s*(\[[^\]]+\]|[^,\n]+),", body)]
        cf = cs[cname]
        assert [n for n, _ in fields] == [n for n, _, _ in cf] == [n for n, _ in ctype._fields_], rname
        for (n, rt), (_, ct, count), (_, pt) in zip(fields, cf, ctype._fields_):
            m = re.match(r"\[(\w+); (\d+)\]$", rt)
            scalar, rcount = (m.group(1), int(m.group(2))) if m else (rt, None)
            assert base.SCALARS[scalar][0] == ct and rcount == count, f"{rname}.{n}: Rust {rt}, C `{ct}`[{count}]"
            assert base.SCALARS[scalar][1] * (count or 1) == C.sizeof(pt), f"{rname}.{n}"
        # every field is naturally aligned with no padding between them, so #[repr(C)] and C agree when the sizes add up
        assert sum(C.sizeof(pt) for _, pt in ctype._fields_) == C.sizeof(ctype), rname
    assert (C.sizeof(_capi.FlacEncodeOptions), C.sizeof(_capi.FlacEncodeRecord)) == (16, 104)


def test_constants_equal_the_headers():
    hdr = HEADER.read_text()
    c_vals = {n: int(v, 0) for n, v in re.findall(r"#define\s+RG_(FLAC_ENC_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", hdr)}
    rust = {n: int(v.replace("_", ""), 0) for n, v in re.findall(r"pub const (FLAC_ENC_\w+):\s*(?:u32|usize)\s*=\s*(0x[0-9A-Fa-f_]+|\d+);", _module())}
    assert len(rust) == 8 and set(rust) == set(c_vals)
    for n, v in rust.items():
        assert c_vals[n] == v, n
        assert getattr(_capi, n) == v, n
    body = re.search(r"impl Default for RgFlacEncodeOptions \{(.*?)\n    \}", _module(), flags=re.S).group(1)
    assert ("block_size", "FLAC_ENC_DEFAULT_BLOCK") in re.findall(r"(\w+): (\w+),", body) and ("flags", "FLAC_ENC_VERIFY") in re.findall(r"(\w+): (\w+),", body)
