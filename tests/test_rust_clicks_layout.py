"""The `clicks` module of the Rust binding (bindings/rust/src/lib.rs) against include/mp3rgain_amd_clicks.h -- without a Rust
toolchain, with the parsers of tests/test_rust_binding_layout.py: the extern declaration of the file call against its prototype,
every #[repr(C)] struct against the C struct's field names, order and types, its size and its fields' offsets against ctypes' of
the same struct, and the constants against the header's."""
import ctypes as C
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import test_rust_binding_layout as base  # noqa: E402
import test_rust_tempo_layout as tempo  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

HEADER = base.ROOT / "include" / "mp3rgain_amd_clicks.h"
STRUCTS = {"RgClicksOpts": ("rg_clicks_opts", _capi.ClicksOpts), "RgClicksChannel": ("rg_clicks_channel", _capi.ClicksChannel),
           "RgClicksEvent": ("rg_clicks_event", _capi.ClicksEvent), "RgClicksResult": ("rg_clicks_result", _capi.ClicksRecord)}
ARRAY = ("[RgClicksChannel; CK_MAX_CHANNELS]", "rg_clicks_channel", "ch[RG_CK_MAX_CHANNELS]")  # the one field that is not a scalar


def _module():
    src = base.rust_source()
    return src[src.index("pub mod clicks {"):src.index("pub mod flacenc {")]


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
    assert set(protos) == {"rg_clicks", "rg_clicks_arena", "rg_clicks_kernel_shape", "rg_clicks_rate"}
    block = re.search(r'extern "C" \{(.*?)\n    \}', _module(), flags=re.S).group(1)
    ext = re.findall(r"pub fn (\w+)\((.*?)\)\s*->\s*([^;]+?)\s*;", block, flags=re.S)
    assert [n for n, _, _ in ext] == ["rg_clicks"]  # the seams and the measurement hook are the tests' and the tools'
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
        assert [n for n, _ in fields] == [n.split("[")[0] for n, _ in cf] == [n for n, _ in ctype._fields_], rname
        offset = 0
        for (n, rt), (cn, ct), (_, pt) in zip(fields, cf, ctype._fields_):
            if rt == ARRAY[0]:
                assert (ct, cn) == ARRAY[1:] and C.sizeof(pt) == _capi.CK_MAX_CHANNELS * C.sizeof(_capi.ClicksChannel), f"{rname}.{n}"
            else:
                assert base.SCALARS[rt][0] == ct, f"{rname}.{n}: Rust {rt}, C `{ct}`"
                assert base.SCALARS[rt][1] == C.sizeof(pt), f"{rname}.{n}"
            # every field is naturally aligned with no padding in front of it, so #[repr(C)], C and ctypes agree on its offset
            assert getattr(ctype, n).offset == offset and offset % C.alignment(pt) == 0, f"{rname}.{n}"
            offset += C.sizeof(pt)
        assert offset == C.sizeof(ctype), rname
    assert [C.sizeof(t) for _, t in STRUCTS.values()] == [28, 40, 20, 400]
    assert (_capi.ClicksRecord.nonfinite.offset, _capi.ClicksRecord.events.offset, _capi.ClicksRecord.ch.offset) == (64, 72, 80)
    # the sizes the header's comments state
    hdr = HEADER.read_text()
    assert "rg_clicks_channel;             /* 40 bytes */" in hdr and "rg_clicks_event;               /* 20 bytes */" in hdr and "= 400 bytes */" in hdr


def test_constants_equal_the_headers():
    hdr = HEADER.read_text()
    c_vals = {n: int(v, 0) for n, v in re.findall(r"#define\s+RG_(CK_\w+)\s+(0x[0-9A-Fa-f]+|\d+)u\b", hdr)}
    rust = {n: int(v.replace("_", ""), 0) for n, v in re.findall(r"pub const (CK_\w+):\s*(?:u32|usize)\s*=\s*(0x[0-9A-Fa-f_]+|\d+);", _module())}
    assert len(rust) == 18 and set(rust) == set(c_vals)
    for n, v in rust.items():
        assert c_vals[n] == v, n
        assert getattr(_capi, n) == v, n
    # the Default of the options is the header's
    body = re.search(r"impl Default for RgClicksOpts \{(.*?)\n    \}", _module(), flags=re.S).group(1)
    assert re.findall(r"(\w+): (\w+),", body) == [("block_samples", "CK_DEFAULT_BLOCK"), ("order", "CK_DEFAULT_ORDER"), ("ratio_permille", "CK_DEFAULT_RATIO_PERMILLE"),
                                                  ("floor", "CK_DEFAULT_FLOOR"), ("gap", "CK_DEFAULT_GAP"), ("max_width", "CK_DEFAULT_MAX_WIDTH"),
                                                  ("max_events", "CK_DEFAULT_MAX_EVENTS")]
