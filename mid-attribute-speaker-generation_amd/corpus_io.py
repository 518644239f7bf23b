"""The two file formats a raw corpus comes in, read on the host without ``librosa``,
``soundfile`` or ``tgt`` (none of them a dependency of this package):

  read_wav        what ``librosa.load(path, sr=None, mono=True)`` decodes (preprocessor.py:186;
                  the resampling that call also does is ``audio.Resampler``, on the device)
  read_textgrid   what ``tgt.io.read_textgrid`` reads (preprocessor.py:177), as plain tuples
"""
import re
import struct

import numpy as np

_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def read_wav(path):
    """A RIFF/WAVE file -> ``(float32 mono samples, sampling rate)``.  PCM of 8 (offset binary),
    16, 24 and 32 bits scaled by ``1 / 2^(bits - 1)``, IEEE float32, and
    ``WAVE_FORMAT_EXTENSIBLE`` of either kind; channels are averaged as
    ``librosa.load(mono=True)`` does.  Chunks before ``data`` are skipped (with the pad byte of
    an odd size); a ``data`` chunk cut short is read up to the bytes present (whole frames).
    Anything else malformed raises ``ValueError`` naming the file."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b"RIFF" or raw[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        tag, size = raw[pos:pos + 4], struct.unpack_from("<I", raw, pos + 4)[0]
        body = raw[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            if len(body) < 16:
                raise ValueError(f"{path}: fmt chunk of {len(body)} bytes")
            fmt = body
        elif tag == b"data":
            data = body  # a truncated file gives the bytes present
            break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: no {'fmt' if fmt is None else 'data'} chunk")
    kind, channels, sr, _, align, bits = struct.unpack_from("<HHIIHH", fmt)
    if kind == _EXTENSIBLE:
        if len(fmt) < 40:
            raise ValueError(f"{path}: extensible fmt chunk of {len(fmt)} bytes")
        kind = struct.unpack_from("<H", fmt, 24)[0]  # the first two bytes of the sub-format GUID
    if channels < 1 or sr < 1:
        raise ValueError(f"{path}: {channels} channels at {sr} Hz")
    width = bits // 8
    if (kind, bits) not in ((_PCM, 8), (_PCM, 16), (_PCM, 24), (_PCM, 32), (_FLOAT, 32)):
        raise ValueError(f"{path}: format tag {kind} with {bits} bits is not read")
    frames = len(data) // (width * channels)
    b = np.frombuffer(data, np.uint8, frames * channels * width)
    if kind == _FLOAT:
        x = b.view("<f4").astype(np.float32)
    elif bits == 8:
        x = (b.astype(np.float32) - 128.0) / 128.0
    elif bits == 16:
        x = b.view("<i2").astype(np.float32) / 32768.0
    elif bits == 32:
        x = (b.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    else:  # 24 bits: the three bytes into the top of an int32
        q = b.reshape(-1, 3).astype(np.int32)
        v = ((q[:, 0] << 8) | (q[:, 1] << 16) | (q[:, 2] << 24)) >> 8
        x = v.astype(np.float32) / 8388608.0
    if channels > 1:
        x = x.reshape(frames, channels).mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(x, np.float32), int(sr)


_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"
_TOKEN = re.compile(r'"((?:[^"]|"")*)"|\[[^\]"]*\]|(' + _NUM + r")|(<exists>|<absent>)")


def read_textgrid(path, include_empty_intervals=False):
    """A Praat TextGrid (long or short text format, UTF-8 with or without a byte-order mark) ->
    ``{tier name: [(start, end, text), ...]}`` for its interval tiers; a point tier is skipped.
    ``""`` inside a text is one quote.  Intervals with empty (or all-blank) text are dropped unless
    ``include_empty_intervals``: that is what ``tgt.io.read_textgrid`` does in the reference
    (tgt 1.4.4), and why the ``''`` entry of its ``sil_phones`` never fires there."""
    with open(path, "rb") as f:
        raw = f.read()
    try:
        text = raw.decode("utf-8-sig")
    except UnicodeDecodeError:
        raise ValueError(f"{path}: not UTF-8") from None
    # the long format labels every value (`xmin = 0`, `intervals [1]:`); only quoted strings,
    # numbers outside `[..]` and the <exists> flag carry data, in the short format's order
    tok = []
    for m in _TOKEN.finditer(text):
        if m.group(1) is not None:
            tok.append(m.group(1).replace('""', '"'))
        elif m.group(2) is not None:
            tok.append(float(m.group(2)))
        elif m.group(3) is not None:
            tok.append(m.group(3))
    try:
        if tok[0] != "ooTextFile" or tok[1] != "TextGrid":
            raise ValueError
        if tok[4] != "<exists>":
            return {}
        n_tiers, pos, tiers = int(tok[5]), 6, {}
        for _ in range(n_tiers):
            kind, name, n = tok[pos], tok[pos + 1], int(tok[pos + 4])
            pos += 5
            if kind == "IntervalTier":
                rows = []
                for _ in range(n):
                    s, e, label = tok[pos:pos + 3]
                    if not isinstance(label, str):
                        raise ValueError
                    pos += 3
                    if label.strip() != "" or include_empty_intervals:
                        rows.append((float(s), float(e), label))
                tiers[name] = rows
            elif kind == "TextTier":
                pos += 2 * n
            else:
                raise ValueError
        return tiers
    except (IndexError, ValueError, TypeError):
        raise ValueError(f"{path}: not a TextGrid this reader understands") from None
