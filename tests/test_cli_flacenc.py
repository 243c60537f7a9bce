"""`--encode` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the
text, TSV and JSON shapes on records the serial twin (rg_flac_encode_arena, route 0) computes, handed to the command in place of
the GPU's."""
import io
import json
from pathlib import Path

import numpy as np
import pytest

from mp3rgain_amd import cli
from mp3rgain_amd import replaygain as rg


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--encode", "--encode-dir", "d", "--encode-lpc", "12", "--encode-block", "512", "--no-encode-verify", "-o", "json", "a.wav"],
                       io.StringIO(), io.StringIO())
    assert (o.encode, str(o.encode_dir), o.encode_lpc, o.encode_block, o.encode_verify, o.output_format) == (True, "d", 12, 512, False, "json")
    o = cli.parse_args(["--encode", "--encode-dir", "d", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.encode_lpc, o.encode_block, o.encode_verify) == (None, None, True)
    for args, text in ((["--encode", "a.wav"], "--encode requires --encode-dir"), (["--encode-dir", "d", "a.wav"], "--encode-dir requires --encode"),
                       (["--encode-lpc", "4", "a.wav"], "--encode-lpc requires --encode"), (["--no-encode-verify", "a.wav"], "requires --encode"),
                       (["--encode", "--encode-dir", "d", "--encode-lpc", "13", "a.wav"], "0 to 12"),
                       (["--encode", "--encode-dir", "d", "--encode-block", "1000", "a.wav"], "256, 512, 1024, 2048 or 4096"),
                       (["--encode", "--encode-dir", "d", "--encode-lpc", "x", "a.wav"], "invalid LPC order: x"),
                       (["--encode", "--encode-dir", "d", "--stereo", "a.wav"], "cannot be combined with --stereo"),
                       (["--encode", "--encode-dir", "d", "--verify", "a.wav"], "--verify"), (["--encode", "--encode-dir", "d", "-r", "a.wav"], "-r"),
                       (["--encode", "--encode-dir", "d", "-a", "a.wav"], "-a"), (["--encode", "--encode-dir", "d", "--rip", "a.wav"], "--rip")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--encode", "--encode-dir")
    assert code == 1 and "--encode-dir requires an argument" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--encode " in out.getvalue() and "--encode-dir <DIR>" in out.getvalue() and "--no-encode-verify" in out.getvalue()


class _TwinAnalyzer:
    """Analyzer.encode_flac from the serial twin: named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def encode_flac(self, files, out_files, block_size=None, max_lpc_order=None, verify=True):
        type(self).seen.append((block_size, max_lpc_order, verify))
        res = []
        for f, dst in zip(files, out_files):
            if str(f) not in self.planes:
                res.append(rg.FlacEncoded(*([0] * 12), bytes(16), bytes(16), 0, rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            streams, recs, _ = rg.flac_encode_arena(None, 0, list(descs)[:1], [16], arena, block_size, max_lpc_order)
            Path(dst).write_bytes(streams[0])
            r = recs[0]
            flags = int(r.flags) | rg._capi.FLAC_ENC_WRITTEN | (rg._capi.FLAC_ENC_VERIFIED if verify else 0)
            res.append(rg.FlacEncoded(int(r.pcm_frames), int(r.flac_frames), 0, int(r.sample_rate), int(r.channels), int(r.bits_per_sample), int(r.block_size),
                                      int(r.min_frame_bytes), int(r.max_frame_bytes), int(r.pcm_bytes), int(r.stream_bytes), int(r.metadata_bytes),
                                      bytes(r.md5_pcm), bytes(r.md5_pcm) if verify else bytes(16), flags, None))
        return res


@pytest.fixture()
def twin(monkeypatch):
    rng = np.random.default_rng(5)
    x = np.cumsum(rng.integers(-300, 300, size=6000)).clip(-30000, 30000).astype(np.int16)
    _TwinAnalyzer.planes = {"a.wav": ([x, (x // 2).astype(np.int16)], 44100), "b.wav": ([x], 48000)}
    _TwinAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _TwinAnalyzer)
    return _TwinAnalyzer


def test_text_tsv_and_json(twin, tmp_path):
    code, out, err = _run("--encode", "--encode-dir", tmp_path, "a.wav", "nothing.wav", "b.wav")
    lines = out.split("\n")
    assert code == 1 and "nothing.wav - Failed to open" in err
    assert lines[0].startswith("mp3rgain encoding 3 file(s) to FLAC in") and f"a.wav -> {tmp_path / 'a.flac'}  " in lines[2] and lines[2].endswith("% of the PCM, verified")
    sizes = [(tmp_path / n).stat().st_size for n in ("a.flac", "b.flac")]
    assert f"{sizes[0]} bytes" in lines[2] and f"2 of 3 file(s) written: {sum(sizes)} bytes" in out and f"of {6000 * 6} bytes of PCM" in out
    assert twin.seen == [(None, None, True)]
    d2 = tmp_path / "two"
    d2.mkdir()
    code, out, _ = _run("--encode", "--encode-dir", d2, "--encode-lpc", "4", "--encode-block", "256", "--no-encode-verify", "-o", "json", "a.wav")
    doc = json.loads(out)
    f = doc["files"][0]
    assert code == 0 and twin.seen[-1] == (256, 4, False) and f["output"] == str(d2 / "a.flac") and f["verified"] is False and f["block_size"] == 256
    assert f["ratio"] == f["stream_bytes"] / f["pcm_bytes"] and doc["pcm_bytes"] == 24000 and doc["summary"]["failed"] == 0 and len(f["md5"]) == 32
    d3 = tmp_path / "three"
    d3.mkdir()
    code, out, _ = _run("--encode", "--encode-dir", d3, "-o", "tsv", "b.wav", "nothing.wav")
    rows = [r.split("\t") for r in out.rstrip("\n").split("\n")]
    assert code == 1 and rows[0][:2] == ["b.wav", str(d3 / "b.flac")] and rows[0][5:9] == [str(-(-6000 // 4096)), "48000", "1", "16"] and rows[1][0] == "nothing.wav"
