"""The two file formats a raw corpus comes in, read on the host without ``librosa``,
``soundfile`` or ``tgt`` (none of them a dependency of this package):

  read_wav        what ``librosa.load(path, sr=None, mono=True)`` decodes (preprocessor.py:186;
                  the resampling that call also does is ``audio.Resampler``, on the device)
  read_textgrid   what ``tgt.io.read_textgrid`` reads (preprocessor.py:177), as plain tuples
  write_textgrid  one interval tier from frame durations (``align.py``), read back exactly
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


def boundary_time(n_frames, hop, sr):
    """The time written for a boundary after ``n_frames`` frames: half a sample past
    ``n_frames * hop / sr``.  The plain quotient does not survive the trip through its decimal
    text and ``int(sr * t)``: for hop 256 at 22 050 Hz, 326 of the boundaries 1..3999 come back one
    sample short, which leaves the trimmed waveform one frame short of its durations.  With the
    half sample ``int(sr * t)`` is ``n_frames * hop`` and ``round(t * sr / hop)`` is ``n_frames``
    whatever way the last bit rounds."""
    return (int(n_frames) * int(hop) + 0.5) / float(sr)


def write_textgrid(path, phones, durations, hop, sr, tier="phones"):
    """Write a long-format TextGrid with one interval tier: phone ``i`` lasts ``durations[i]``
    frames of ``hop`` samples at ``sr``, boundaries at ``boundary_time``.  ``read_textgrid``,
    ``preprocess.durations_from_intervals`` and the trim ``int(sr * start):int(sr * end)`` give
    back these durations and a waveform of ``sum(durations) * hop`` samples (leading and trailing
    silence phones are trimmed there as for any TextGrid)."""
    phones, durations = list(phones), [int(d) for d in durations]
    if len(phones) != len(durations) or not phones:
        raise ValueError(f"{path}: {len(phones)} phones and {len(durations)} durations")
    if any(d < 0 for d in durations) or any(str(p).strip() == "" for p in phones):
        raise ValueError(f"{path}: a negative duration or an empty phone")
    edges = [0]
    for d in durations:
        edges.append(edges[-1] + d)
    times = [repr(boundary_time(n, hop, sr)) for n in edges]
    lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0",
             f"xmax = {times[-1]}", "tiers? <exists>", "size = 1", "item []:", "    item [1]:",
             '        class = "IntervalTier"', '        name = "' + tier.replace('"', '""') + '"',
             "        xmin = 0", f"        xmax = {times[-1]}",
             f"        intervals: size = {len(phones)}"]
    for i, p in enumerate(phones):
        lines += [f"        intervals [{i + 1}]:", f"            xmin = {times[i]}",
                  f"            xmax = {times[i + 1]}",
                  '            text = "' + str(p).replace('"', '""') + '"']
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
