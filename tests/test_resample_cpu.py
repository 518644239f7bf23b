"""The host side of corpus building: the resampler's oracle against scipy and its filter's
quality (resample_oracle.py), ``corpus_io.read_wav`` / ``read_textgrid`` on files written here,
and the split arithmetic of ``preprocess.write_split``.  No GPU.
"""
import importlib
import math
import struct
import wave

import numpy as np
import pytest

import resample_oracle as O

NAME = "mid-attribute-speaker-generation_amd"
SR_OUT = 22050


def _mod(name):
    return importlib.import_module(f"{NAME}.{name}")


# ------------------------------------------------------------------ the filter and the oracle
@pytest.mark.parametrize("sr_in", (48000, 24000, 16000, 44100, 11025))
def test_oracle_matches_scipy_and_filter_is_the_oracles(sr_in):
    from scipy.signal import resample_poly
    h, L, M, half = O.design(sr_in, SR_OUT)
    assert (L, M) == O.ratio(sr_in, SR_OUT) and math.gcd(L, M) == 1 and len(h) == 2 * half + 1
    x = 0.3 * np.random.default_rng(sr_in).standard_normal(700)
    got = O.oracle64(x, sr_in, SR_OUT, table=L * h)
    want = resample_poly(x, L, M, window=h, padtype="constant")  # scipy scales by L itself
    assert len(got) == len(want) == O.n_out(700, L, M) == -(-700 * L // M)
    dev = np.abs(got - want).max()
    print(f"{sr_in}: L {L} M {M} half {half} oracle64 vs scipy {dev:.2e}")
    assert dev <= 1e-12
    table, L2, M2, half2 = _mod("audio").resample_filter(sr_in, SR_OUT)
    assert (L2, M2, half2) == (L, M, half) and table.dtype == np.float32
    assert np.array_equal(table, O.table32(sr_in, SR_OUT)[0])
    assert np.array_equal(table, (L * h).astype(np.float32))


def _tone(sr, hz, n, phase=0.3):
    return np.sin(2.0 * np.pi * hz * np.arange(n) / sr + phase)


@pytest.mark.parametrize("sr_in", (48000, 24000, 44100, 16000))
def test_filter_quality_float64(sr_in):
    h, L, M, half = O.design(sr_in, SR_OUT)
    n = 6000
    n_out = O.n_out(n, L, M)
    mid = slice(n_out // 4, 3 * n_out // 4)
    nyq = min(sr_in, SR_OUT) / 2.0
    for hz in (1000.0, 0.8 * nyq):
        y = O.oracle64(_tone(sr_in, hz, n), sr_in, SR_OUT, table=L * h)
        dev = np.abs(y - _tone(SR_OUT, hz, n_out))[mid].max()
        print(f"{sr_in}: passband {hz:.0f} Hz dev {dev:.2e}")
        assert dev <= 1e-6
    if sr_in > SR_OUT:  # what would alias is gone
        y = O.oracle64(_tone(sr_in, 1.15 * SR_OUT / 2.0, n), sr_in, SR_OUT, table=L * h)
        rms = float(np.sqrt(np.mean(y[mid] ** 2)))
        print(f"{sr_in}: stopband rms {rms:.2e}")
        assert rms < 1e-6


def test_ref32_is_the_definition_in_float32():
    x = (0.3 * np.random.default_rng(1).standard_normal(700)).astype(np.float32)
    for sr_in in (48000, 11025):
        dev = np.abs(O.ref32(x, sr_in, SR_OUT) - O.oracle64(x, sr_in, SR_OUT)).max()
        assert 0.0 < dev < 2e-6


# ------------------------------------------------------------------ read_wav
def _riff(fmt_body, data, before=b"", data_size=None):
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt_body)) + fmt_body + before
    body += b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _fmt(kind, channels, sr, bits):
    align = channels * bits // 8
    return struct.pack("<HHIIHH", kind, channels, sr, sr * align, align, bits)


def _fmt_ext(kind, channels, sr, bits):
    guid = struct.pack("<H", kind) + bytes.fromhex("000000001000800000aa00389b71")
    return _fmt(0xFFFE, channels, sr, bits) + struct.pack("<HHI", 22, bits, 0) + guid


def _chunk(tag, payload):
    return tag + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")


def test_read_wav_16_bit_through_the_wave_module(tmp_path):
    read_wav = _mod("corpus_io").read_wav
    rng = np.random.default_rng(2)
    mono = rng.integers(-32768, 32768, 301).astype("<i2")
    mono[:2] = (-32768, 32767)
    stereo = rng.integers(-32768, 32768, (200, 2)).astype("<i2")
    for name, a, ch, sr in (("m.wav", mono, 1, 24000), ("s.wav", stereo, 2, 48000)):
        with wave.open(str(tmp_path / name), "wb") as w:
            w.setnchannels(ch), w.setsampwidth(2), w.setframerate(sr)
            w.writeframes(a.tobytes())
    x, sr = read_wav(str(tmp_path / "m.wav"))
    assert sr == 24000 and x.dtype == np.float32 and x.shape == (301,)
    assert np.array_equal(x, mono.astype(np.float32) / 32768.0)
    x, sr = read_wav(str(tmp_path / "s.wav"))
    assert sr == 48000 and x.shape == (200,)
    assert np.array_equal(x, (stereo.astype(np.float32) / 32768.0).mean(axis=1, dtype=np.float32))


def test_read_wav_hand_packed_formats(tmp_path):
    read_wav = _mod("corpus_io").read_wav
    rng = np.random.default_rng(3)

    def roundtrip(name, blob):
        p = tmp_path / name
        p.write_bytes(blob)
        return read_wav(str(p))

    v24 = np.concatenate([[-(1 << 23), (1 << 23) - 1, -1, 0, 1], rng.integers(-(1 << 23), 1 << 23, 50)])
    b24 = b"".join(struct.pack("<i", int(v))[:3] for v in v24)
    x, sr = roundtrip("p24.wav", _riff(_fmt(1, 1, 44100, 24), b24))
    assert sr == 44100 and np.array_equal(x, v24.astype(np.float32) / 8388608.0)

    v32 = np.concatenate([[-(1 << 31), (1 << 31) - 1], rng.integers(-(1 << 31), 1 << 31, 50)])
    x, _ = roundtrip("p32.wav", _riff(_fmt(1, 1, 16000, 32), v32.astype("<i4").tobytes()))
    assert np.array_equal(x, (v32.astype(np.float64) / 2147483648.0).astype(np.float32))

    v8 = np.r_[np.arange(0, 250, 5), 255].astype(np.uint8)  # offset binary; 51 bytes: an odd-sized data chunk
    x, _ = roundtrip("p8.wav", _riff(_fmt(1, 1, 8000, 8), v8.tobytes()))
    assert len(v8) & 1 and np.array_equal(x, (v8.astype(np.float32) - 128.0) / 128.0)

    f = rng.standard_normal(64).astype("<f4")
    x, _ = roundtrip("f32.wav", _riff(_fmt(3, 1, 48000, 32), f.tobytes()))
    assert np.array_equal(x, f)
    f2 = rng.standard_normal((40, 2)).astype("<f4")  # extensible float, stereo, a fact chunk
    x, sr = roundtrip("xf.wav", _riff(_fmt_ext(3, 2, 48000, 32), f2.tobytes(),
                                      before=_chunk(b"fact", struct.pack("<I", 40))))
    assert sr == 48000 and np.array_equal(x, f2.mean(axis=1, dtype=np.float32))
    v16 = rng.integers(-32768, 32768, 33).astype("<i2")
    x, _ = roundtrip("x16.wav", _riff(_fmt_ext(1, 1, 22050, 16), v16.tobytes()))
    assert np.array_equal(x, v16.astype(np.float32) / 32768.0)

    # a LIST chunk of odd size (pad byte) before data
    x, _ = roundtrip("list.wav", _riff(_fmt(1, 1, 22050, 16), v16.tobytes(),
                                       before=_chunk(b"LIST", b"INFOISFT\x03\0\0\0abc")))
    assert np.array_equal(x, v16.astype(np.float32) / 32768.0)
    # a data chunk that promises more than the file holds: the whole frames present
    x, _ = roundtrip("cut.wav", _riff(_fmt(1, 1, 22050, 16), v16.tobytes()[:41], data_size=4000))
    assert np.array_equal(x, v16[:20].astype(np.float32) / 32768.0)


def test_read_wav_rejects_what_it_cannot_read(tmp_path):
    read_wav = _mod("corpus_io").read_wav
    cases = {"text.wav": b"this is not a wave file at all",
             "nofmt.wav": b"RIFF" + struct.pack("<I", 12) + b"WAVE" + _chunk(b"data", b"\0\0"),
             "nodata.wav": b"RIFF" + struct.pack("<I", 28) + b"WAVE" + _chunk(b"fmt ", _fmt(1, 1, 8000, 16)),
             "adpcm.wav": _riff(_fmt(2, 1, 8000, 4), b"\0" * 8)}
    for name, blob in cases.items():
        p = tmp_path / name
        p.write_bytes(blob)
        with pytest.raises(ValueError, match=name):
            read_wav(str(p))


# ------------------------------------------------------------------ read_textgrid
PHONES = [(0.0, 0.05, "sil"), (0.05, 0.12, "a"), (0.12, 0.2, ""), (0.2, 0.33, 'o"q'),
          (0.33, 0.33, "k"), (0.33, 0.4, "sp"), (0.4, 0.52, "i"), (0.52, 0.6, "sil")]
WORDS = [(0.0, 0.05, ""), (0.05, 0.52, "ao ki"), (0.52, 0.6, "")]
POINTS = [(0.1, "p1"), (0.3, "p 2")]


def _q(s):
    return '"' + s.replace('"', '""') + '"'


def long_textgrid(tiers, xmax, points=None):
    """Praat's long text format of interval tiers ``{name: rows}`` (and one point tier)."""
    n = len(tiers) + (points is not None)
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", f"xmax = {xmax}",
           "tiers? <exists>", f"size = {n}", "item []:"]
    k = 0
    for name, rows in tiers.items():
        k += 1
        out += [f"    item [{k}]:", '        class = "IntervalTier"', f"        name = {_q(name)}",
                "        xmin = 0", f"        xmax = {xmax}", f"        intervals: size = {len(rows)}"]
        for i, (s, e, t) in enumerate(rows, 1):
            out += [f"        intervals [{i}]:", f"            xmin = {s!r}", f"            xmax = {e!r}",
                    f"            text = {_q(t)}"]
        if points is not None and k == 1:  # the point tier sits between the interval tiers
            k += 1
            out += [f"    item [{k}]:", '        class = "TextTier"', '        name = "marks"',
                    "        xmin = 0", f"        xmax = {xmax}", f"        points: size = {len(points)}"]
            for i, (t, m) in enumerate(points, 1):
                out += [f"        points [{i}]:", f"            number = {t!r}", f"            mark = {_q(m)}"]
    return "\n".join(out) + "\n"


def short_textgrid(tiers, xmax, points=None):
    n = len(tiers) + (points is not None)
    out = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "0", f"{xmax}", "<exists>", f"{n}"]
    first = True
    for name, rows in tiers.items():
        out += ['"IntervalTier"', _q(name), "0", f"{xmax}", f"{len(rows)}"]
        for s, e, t in rows:
            out += [repr(s), repr(e), _q(t)]
        if points is not None and first:
            out += ['"TextTier"', '"marks"', "0", f"{xmax}", f"{len(points)}"]
            for t, m in points:
                out += [repr(t), _q(m)]
        first = False
    return "\n".join(out) + "\n"


def test_read_textgrid_long_and_short(tmp_path):
    read_textgrid = _mod("corpus_io").read_textgrid
    tiers = {"phones": PHONES, "words": WORDS}
    (tmp_path / "long.TextGrid").write_text(long_textgrid(tiers, 0.6, POINTS), encoding="utf-8")
    (tmp_path / "short.TextGrid").write_bytes(b"\xef\xbb\xbf" + short_textgrid(tiers, 0.6, POINTS).encode())
    got = [read_textgrid(str(tmp_path / f"{n}.TextGrid")) for n in ("long", "short")]
    assert got[0] == got[1]
    assert list(got[0]) == ["phones", "words"]  # the point tier is skipped
    assert got[0]["phones"] == [r for r in PHONES if r[2] != ""]  # tgt's default: empties dropped
    assert got[0]["phones"][2][2] == 'o"q' and got[0]["words"] == [WORDS[1]]
    full = read_textgrid(str(tmp_path / "long.TextGrid"), include_empty_intervals=True)
    assert full == {"phones": PHONES, "words": WORDS}
    assert full == read_textgrid(str(tmp_path / "short.TextGrid"), include_empty_intervals=True)
    (tmp_path / "bad.TextGrid").write_text("xmin = 0\nxmax = 1\n")
    with pytest.raises(ValueError, match="bad.TextGrid"):
        read_textgrid(str(tmp_path / "bad.TextGrid"))


def test_read_textgrid_feeds_durations_from_intervals(tmp_path):
    PRE = _mod("preprocess")
    (tmp_path / "a.TextGrid").write_text(long_textgrid({"phones": PHONES}, 0.6), encoding="utf-8")
    tier = _mod("corpus_io").read_textgrid(str(tmp_path / "a.TextGrid"))["phones"]
    direct = PRE.durations_from_intervals([r for r in PHONES if r[2] != ""], 22050, 256)
    assert PRE.durations_from_intervals(tier, 22050, 256) == direct
    phones, durations, start, end = direct
    assert phones == ["a", 'o"q', "k", "sp", "i"] and durations[2] == 0 and (start, end) == (0.05, 0.52)


# ------------------------------------------------------------------ the split
def _lines():
    return [[f"a{i:02d}|spkA|{{a}}|text" for i in range(7)], [f"b{i:02d}|spkB|{{o}}|text" for i in range(10)]]


def test_split_arithmetic(tmp_path):
    PRE = _mod("preprocess")
    val = test = 0.2
    dirs = [tmp_path / n for n in ("one", "two", "three")]
    for d in dirs:
        d.mkdir()
    out = PRE.write_split(_lines(), str(dirs[0]), val, test, seed=7)
    read = lambda d: {n: (d / f"{n}.txt").read_text(encoding="utf-8").splitlines()  # noqa: E731
                      for n in ("train", "val", "test")}
    parts = read(dirs[0])
    everything = [m for spk in _lines() for m in spk]
    joined = parts["train"] + parts["val"] + parts["test"]
    assert sorted(joined) == sorted(everything) and len(set(joined)) == len(everything)
    assert sorted(m for spk in out for m in spk) == sorted(everything)
    for tag, n in (("spkA", 7), ("spkB", 10)):
        a, b = int(n * (1 - val - test)), int(n * (1 - test))
        count = {k: sum(tag in m for m in v) for k, v in parts.items()}
        assert count == {"train": a, "val": b - a, "test": n - b}
    PRE.write_split(_lines(), str(dirs[1]), val, test, seed=7)
    assert read(dirs[1]) == parts
    PRE.write_split(_lines(), str(dirs[2]), val, test, seed=8)
    assert read(dirs[2]) != parts
