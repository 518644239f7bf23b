"""Objective synthesis metrics on the device: does what the model synthesises resemble the
recording?  (the kernels are in ``csrc/metrics.hip``.)

Free-running synthesis predicts its own durations, so a synthesised mel and the recorded one have
different lengths and cannot be compared frame by frame.  Both are turned into MFCCs, aligned by
dynamic time warping (``fs2_dtw``), and ``fs2_path_metrics`` writes one fp64 record per pair along
the alignment path.  Everything stays on the device; ``summarise`` makes the one host read.

**What the MCD here is.**  The mel-cepstral distortion reported is the MFCC distortion of THIS
PROJECT'S OWN natural-log mel -- ``log(clamp(mel, 1e-5))`` of ``audio.MelFrontEnd``, the quantity
the model is trained on -- as coefficients 1..K of the orthonormal DCT-II over the mel axis:
``(10 / ln 10) sqrt(2) * mean over the DTW path of ||c_a - c_b||_2`` in dB.  It ranks checkpoints
of one corpus against each other.  No parity with SPTK or WORLD mel-cepstra is claimed, and the
numbers are not comparable with MCDs published from those.  The DTW steps are the three unit steps
(the defaults of ``librosa.sequence.dtw``); librosa is not a dependency and no parity with it is
claimed either."""
import math

import numpy as np
import torch

from . import kernels as K

# the fields of a record, in order (fs2_path_metrics)
FIELDS = ("path_len", "mcd_db", "frames_a", "frames_b", "n_vv", "f0_sq_cents", "n_vuv", "len_err")
PATH_LEN, MCD_DB, FRAMES_A, FRAMES_B, N_VV, F0_SQ_CENTS, N_VUV, LEN_ERR = range(len(FIELDS))
DVEC_COS = len(FIELDS)  # the extra column ``compare_wavs(..., trainer=)`` appends
assert len(FIELDS) == K.METRIC_FIELDS

_DCT = {}


def dct_table(n_mels, n_coef):
    """(n_mels, n_coef) float32: ``sqrt(2 / n_mels) cos(pi (2 m + 1) k / (2 n_mels))`` for
    k = 1..n_coef -- rows 1..n_coef of the orthonormal DCT-II, transposed -- computed in fp64 and
    rounded once, as ``audio.twiddle_table``."""
    n_mels, n_coef = int(n_mels), int(n_coef)
    if not 1 <= n_coef < n_mels:
        raise ValueError(f"n_coef {n_coef}: 1..n_mels - 1 = {n_mels - 1}")
    m = np.arange(n_mels, dtype=np.float64)[:, None]
    k = np.arange(1, n_coef + 1, dtype=np.float64)[None, :]
    return (np.sqrt(2.0 / n_mels) * np.cos(np.pi * (2.0 * m + 1.0) * k / (2.0 * n_mels))
            ).astype(np.float32)


def _dct_on(device, n_mels, n_coef):
    key = (str(device), int(n_mels), int(n_coef))
    if key not in _DCT:
        _DCT[key] = torch.from_numpy(dct_table(n_mels, n_coef)).to(device)
    return _DCT[key]


def mfcc(logmel, n_frames, n_coef=13, rows=False):
    """log-mel -> cepstral coefficients 1..n_coef (c0, the level, is dropped): logmel
    (B, n_mels, F) as ``MelFrontEnd.__call__`` returns it, or with ``rows`` the model's row
    layout (B, F, n_mels) / (B * F, n_mels); ``n_frames`` device int64 (B), not read back ->
    (B, F, n_coef) f32, zeros at and past ``n_frames``."""
    n_mels = logmel.shape[-1] if rows else logmel.shape[1]
    return K.mfcc(logmel, n_frames, _dct_on(logmel.device, n_mels, n_coef), rows=rows)


def dtw(a, b, la, lb):
    """a (B, T1max, K), b (B, T2max, K) f32 with device int64 lengths -> ``(cost (B) f64, path
    (B, T1max + T2max - 1, 2) int32 from (0, 0) to (la - 1, lb - 1), path_len (B) int32)``.
    fp64 Euclidean local cost, steps (1, 1), (1, 0), (0, 1), the first minimum in that order at a
    tie; padded lengths up to 2048."""
    return K.dtw(a, b, la, lb)


def _lens(lens, device):
    return lens.to(device=device, dtype=torch.int64).contiguous()


def compare_mels(mel_a, len_a, mel_b, len_b, n_coef=13, f0_a=None, f0_b=None, rows=False):
    """MFCCs of both, DTW, the path records -> (B, len(FIELDS)) f64 on the device, no host read.

    ``mel_a`` / ``mel_b``: natural-log mels (B, n_mels, Fa) / (B, n_mels, Fb), or with ``rows``
    (B, Fa, n_mels) / (B, Fb, n_mels) as the model returns them; ``len_a`` / ``len_b``: device
    int64 (B), each at least 1.  ``f0_a`` (B, Fa) / ``f0_b`` (B, Fb): F0 contours on the same
    frames, 0 = unvoiced (``PitchExtractor``); without them the F0 fields are 0."""
    dev = mel_a.device
    la, lb = _lens(len_a, dev), _lens(len_b, dev)
    ca = mfcc(mel_a.contiguous().float(), la, n_coef, rows)
    cb = mfcc(mel_b.contiguous().float(), lb, n_coef, rows)
    cost, path, path_len = K.dtw(ca, cb, la, lb)
    if f0_a is not None:
        f0_a, f0_b = f0_a.contiguous().float(), f0_b.contiguous().float()
    return K.path_metrics(cost, path, path_len, la, lb, ca.shape[1], cb.shape[1], f0_a, f0_b)


def compare_wavs(wav_a, lens_a, wav_b, lens_b, front_end, pitch=None, trainer=None):
    """Two batches of waveforms (B, Sa) / (B, Sb) with their sample counts -> the records of
    ``compare_mels`` over ``front_end``'s log-mels; with ``pitch`` (a ``PitchExtractor`` on the
    same hop) YIN contours of both sides fill the F0 fields; with ``trainer`` (an
    ``EmbedderTrainer``) column ``DVEC_COS`` is appended: the cosine similarity of the two
    d-vectors (``dvector_from_wav``) of each pair."""
    mel_a, _, nf_a = front_end(wav_a, lens_a)[:3]
    mel_b, _, nf_b = front_end(wav_b, lens_b)[:3]
    f0_a = f0_b = None
    if pitch is not None:
        if pitch.hop != front_end.hop:
            raise ValueError(f"pitch hop {pitch.hop} is not the front end's {front_end.hop}")
        f0_a, f0_b = pitch(wav_a, lens_a)[0], pitch(wav_b, lens_b)[0]
    rec = compare_mels(mel_a, nf_a, mel_b, nf_b, f0_a=f0_a, f0_b=f0_b)
    if trainer is not None:
        da = trainer.dvector_from_wav(wav_a, lens_a).double()
        db = trainer.dvector_from_wav(wav_b, lens_b).double()
        cos = (da * db).sum(1) / (da.norm(dim=1) * db.norm(dim=1))
        rec = torch.cat([rec, cos[:, None]], dim=1)
    return rec


PER_FIELDS = ("distance", "substitutions", "deletions", "insertions", "phonemes")


def phoneme_error_rate(recognizer, mels, mel_lens, texts, src_lens, rows=False):
    """Intelligibility: the greedy transcription of each mel by ``recognizer`` (a
    ``recognizer.RecognizerTrainer``) against the phonemes ``texts`` (B, T_s) int64 with lengths
    ``src_lens``; mels (B, T, n_mels) in the model's row layout, as the PostNet returns them
    (what they hold past ``mel_lens`` does not matter: the recogniser masks it).
    Everything stays on the device: the int64 sums ``PER_FIELDS`` = [distance, substitutions,
    deletions, insertions, reference phonemes] over the batch, to be added up over a pass and
    given to ``per_from_sums``; with ``rows`` the per-utterance records (B, 4) and the reference
    lengths (B) instead.

    The PER is that of the project's own small recogniser, trained on the same corpus: it compares
    runs that share a recogniser checkpoint, and is no word error rate, no substitute for a
    listening test and nothing across recognisers."""
    dev = mels.device
    sl = _lens(src_lens, dev).clamp(0, texts.shape[1])
    rec = recognizer.errors(mels.contiguous().float(), _lens(mel_lens, dev),
                            texts.to(device=dev, dtype=torch.int64).contiguous(), sl)
    if rows:
        return rec, sl
    return torch.cat([rec.sum(0), sl.sum().reshape(1)])


def per_from_sums(sums):
    """The figures of a pass from the five sums of ``phoneme_error_rate`` (host ints): ``per`` =
    sum of distances / sum of reference lengths (insertions count, so it can exceed 1; nan
    without a reference phoneme) and the parts."""
    out = {k: int(v) for k, v in zip(PER_FIELDS, sums)}
    out["per"] = out["distance"] / out["phonemes"] if out["phonemes"] > 0 else float("nan")
    return out


def from_sums(sums, n):
    """The corpus figures from the column sums of ``n`` records (host floats)."""
    sums = [float(s) for s in sums]
    out = {
        "utterances": int(n),
        "mcd_db": sums[MCD_DB] / n,
        "length_error": sums[LEN_ERR] / n,
        "f0_rmse_cents": math.sqrt(sums[F0_SQ_CENTS] / sums[N_VV]) if sums[N_VV] > 0 else float("nan"),
        "vuv_error": sums[N_VUV] / sums[PATH_LEN],
        "voiced_pairs": sums[N_VV],
        "path_len": sums[PATH_LEN],
    }
    if len(sums) > DVEC_COS:
        out["dvector_cos"] = sums[DVEC_COS] / n
    return out


def summarise(records):
    """records (N, R) -> a dict of floats, with the one host read of the pass: the mean MCD over
    utterances (dB), the mean relative length error (frames_a - frames_b) / frames_b, the F0 RMSE
    ``sqrt(sum f0_sq_cents / sum n_vv)`` in cents (nan without a pair voiced in both), the V/UV
    error ``sum n_vuv / sum path_len`` and, where present, the mean d-vector cosine."""
    if records.dim() != 2 or records.shape[1] < len(FIELDS) or records.shape[0] < 1:
        raise ValueError(f"records are (N >= 1, {len(FIELDS)}[+1]), got {tuple(records.shape)}")
    return from_sums(records.double().sum(0).tolist(), records.shape[0])
