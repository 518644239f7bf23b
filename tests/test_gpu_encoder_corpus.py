"""``embedder_preprocess.EncoderPreprocessor`` on a JVS-layout and a VCTK-layout tree written
here: two speakers each, 24 kHz 16-bit and 48 kHz float32 files of 0.1 - 0.6 s, one file with an
inner gap at floor level (two intervals at ``top_db = 40``, the second too short), files shorter
than ``utter_min_len`` and a speaker who has nothing else.  ``tisv_frame = 8`` and ``batch = 3``,
so a speaker's files span two groups and a group mixes file rates.

No new tolerance: every written file is compared bitwise with the composition of the public
single-utterance pieces on each file alone -- ``Resampler``, ``SilenceSplitter``,
``MelFrontEnd.mel_spectrogram`` of each kept interval, torch slicing by the window rule -- which
checks the batching, the descriptors and the ordering.
"""
import importlib
import os
import struct
import wave

import numpy as np
import pytest
import torch

import pitch_oracle as PO
import vad_oracle as V

NAME = "mid-attribute-speaker-generation_amd"
pytestmark = pytest.mark.gpu

SR, HOP, WINDOW, TISV, TOP_DB = 22050, 256, 1024, 8, 40.0
MIN_LEN = TISV * HOP + WINDOW  # 3072 samples at 22 050 Hz: 0.139 s
# corpus -> speaker -> (gender, [(basename, file rate, format, seconds, glide Hz, gap in seconds)])
GAP = (0.29, 0.465)  # the tail after it, 35 ms, stays below MIN_LEN with its frames
TREE = {
    "jvs": {"jvs001": ("M", [("VOICEACTRESS100_001", 24000, "i16", 0.50, (120.0, 150.0), None),
                             ("VOICEACTRESS100_002", 48000, "f32", 0.40, (200.0, 170.0), None),
                             ("VOICEACTRESS100_003", 24000, "i16", 0.50, (140.0, 180.0), GAP),
                             ("VOICEACTRESS100_004", 48000, "f32", 0.60, (160.0, 210.0), None)]),
            "jvs002": ("F", [("VOICEACTRESS100_001", 24000, "i16", 0.30, (230.0, 190.0), None),
                             ("VOICEACTRESS100_002", 48000, "f32", 0.10, (250.0, 220.0), None)])},
    "vctk": {"p225": ("F", [("p225_001", 48000, "f32", 0.35, (210.0, 240.0), None),
                            ("p225_002", 24000, "i16", 0.45, (190.0, 230.0), None)]),
             "p226": ("M", [("p226_001", 48000, "f32", 0.10, (110.0, 130.0), None),
                            ("p226_002", 24000, "i16", 0.12, (100.0, 120.0), None)])},
}
TEST_SPEAKERS = {"jvs": ["jvs002"], "vctk": []}
NAMES = {"jvs001": "jvs_jvs001_m_jp.npy", "jvs002": "jvs_jvs002_f_jp.npy",
         "p225": "vctk_p225_f_en.npy", "p226": "vctk_p226_m_en.npy"}


def _mod(name):
    return importlib.import_module(f"{NAME}.{name}")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _write_wav(path, x, sr, fmt):
    if fmt == "i16":
        with wave.open(path, "wb") as w:
            w.setnchannels(1), w.setsampwidth(2), w.setframerate(sr)
            w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())
        return
    data = x.astype("<f4").tobytes()
    fmt_body = struct.pack("<HHIIHH", 3, 1, sr, sr * 4, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt_body + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def _wav_path(roots, corpus, spkr, base):
    if corpus == "jvs":
        return os.path.join(roots["jvs"], spkr, "parallel100", "wav24kHz16bit", base + ".wav")
    return os.path.join(roots["vctk"], "wav48", spkr, base + ".wav")


def _alone(path, top_db=TOP_DB):
    """One file through the public single-utterance pieces: ``(windows [(80, TISV) tensors],
    intervals)``."""
    A = _mod("audio")
    x, sr = _mod("corpus_io").read_wav(path)
    y, n = A.Resampler(SR)(_dev(x[None]), None, sr)
    y = y[0, :int(n[0])].contiguous()
    iv, cnt = A.SilenceSplitter(top_db=top_db)(y)
    iv = iv[:int(cnt)].cpu().numpy()
    fe, out = A.MelFrontEnd(), []
    for a, e in iv:
        if e - a < MIN_LEN:
            continue
        mel = fe.mel_spectrogram(y[a:e][None].contiguous())[0]
        assert mel.shape == (80, 1 + (e - a) // HOP)
        out.extend(mel[:, s:s + TISV] for s in V.windows(mel.shape[1], TISV))
    return out, iv


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("encoder_corpus"))
    roots = {"jvs": os.path.join(root, "jvs_ver1"), "vctk": os.path.join(root, "VCTK-Corpus")}
    for c, speakers in TREE.items():
        for spkr, (_, files) in speakers.items():
            for i, (base, sr, fmt, seconds, glide, gap) in enumerate(files):
                path = _wav_path(roots, c, spkr, base)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                n = int(round(seconds * sr))
                x = PO.voice(n, glide[0] * PO.SR / sr, glide[1] * PO.SR / sr, seed=n + i)
                if gap is not None:
                    a, b = int(gap[0] * sr), int(gap[1] * sr)
                    x[a:b] = 1e-4 * np.random.default_rng(1).standard_normal(b - a)
                _write_wav(path, x, sr, fmt)
    with open(os.path.join(roots["jvs"], "gender_f0range.txt"), "w") as f:
        f.write("speaker Male_or_Female minf0[Hz] maxf0[Hz]\njvs001 M 70 300\njvs002 F 130 450\n")
    with open(os.path.join(roots["vctk"], "speaker-info.txt"), "w") as f:
        f.write("ID  AGE  GENDER  ACCENTS  REGION\n225  23  F    English    Southern  England\n"
                "226  22  M    English    Surrey\n")
    EP = _mod("embedder_preprocess")
    corpora = [EP.SpeakerCorpus.jvs(roots["jvs"], TEST_SPEAKERS["jvs"]),
               EP.SpeakerCorpus.vctk(roots["vctk"], TEST_SPEAKERS["vctk"])]
    train, test = os.path.join(root, "train_mel"), os.path.join(root, "test_mel")
    pre = EP.EncoderPreprocessor(corpora, train, test, tisv_frame=TISV, top_db=TOP_DB, batch=3)
    report = pre.save_spectrogram_tisv()
    alone = {}
    for c, speakers in TREE.items():
        for spkr, (_, files) in speakers.items():
            alone[spkr] = [_alone(_wav_path(roots, c, spkr, f[0])) for f in files]
    return {"root": root, "roots": roots, "train": train, "test": test, "report": report,
            "alone": alone, "corpora": corpora, "pre": pre}


def _want(alone, spkr):
    return torch.stack([w for wins, _ in alone[spkr] for w in wins]).cpu().numpy()


def test_the_fixture_is_what_it_says(corpus):
    alone = corpus["alone"]
    wins, iv = alone["jvs001"][2]  # the file with the gap: two intervals, the second too short
    assert len(iv) == 2 and iv[0, 1] - iv[0, 0] >= MIN_LEN and iv[1, 1] - iv[1, 0] < MIN_LEN
    assert len(wins) == 2 * (1 + (iv[0, 1] - iv[0, 0]) // HOP) // TISV - 1
    for spkr in ("jvs001", "p225"):
        assert all(len(w) >= 2 for w, _ in alone[spkr])
    assert [len(w) for w, _ in alone["jvs002"]] == [len(alone["jvs002"][0][0]), 0]
    assert len(alone["jvs002"][0][0]) >= 2
    assert [len(w) for w, _ in alone["p226"]] == [0, 0]
    for spkr in alone:  # the others are one interval, the whole file
        for k, (_, iv) in enumerate(alone[spkr]):
            assert len(iv) == (2 if (spkr, k) == ("jvs001", 2) else 1) and iv[0, 0] == 0


def test_files_are_the_single_utterance_results_bitwise(corpus):
    alone, report = corpus["alone"], corpus["report"]
    assert list(report) == [NAMES[s] for s in ("jvs001", "jvs002", "p225", "p226")]
    assert sorted(os.listdir(corpus["train"])) == sorted([NAMES["jvs001"], NAMES["p225"]])
    assert os.listdir(corpus["test"]) == [NAMES["jvs002"]]  # the test speaker
    for spkr, folder in (("jvs001", "train"), ("p225", "train"), ("jvs002", "test")):
        got = np.load(os.path.join(corpus[folder], NAMES[spkr]))
        want = _want(alone, spkr)
        assert got.dtype == np.float32 and got.shape == want.shape and got.shape[1:] == (80, TISV)
        assert np.array_equal(got, want), spkr
        assert report[NAMES[spkr]] == len(want)
    assert report[NAMES["p226"]] == 0  # nothing long enough: reported, no file


def test_process_wavs_counts_and_the_reference_setting(corpus):
    """Per-file counts; and at top_db = 100 the file with the gap is one interval: whole
    utterance -> mel -> windows."""
    pre, roots = corpus["pre"], corpus["roots"]
    paths = dict(corpus["corpora"][0].spkr_wavlist())["jvs001"]
    windows, counts = pre.process_wavs(paths)
    assert counts == [len(w) for w, _ in corpus["alone"]["jvs001"]] and windows.shape[0] == sum(counts)
    none, counts = pre.process_wavs(dict(corpus["corpora"][1].spkr_wavlist())["p226"])
    assert none.shape == (0, 80, TISV) and counts == [0, 0]
    EP = _mod("embedder_preprocess")
    ref = EP.EncoderPreprocessor([], corpus["train"], corpus["test"], tisv_frame=TISV, batch=3)
    assert ref.splitter.top_db == 100.0
    gap_file = _wav_path(roots, "jvs", "jvs001", "VOICEACTRESS100_003")
    got, counts = ref.process_wavs([gap_file])
    wins, iv = _alone(gap_file, top_db=100.0)
    assert len(iv) == 1 and iv[0].tolist() == [0, 11025] and counts == [len(wins)]
    assert torch.equal(got, torch.stack(wins))
    assert len(wins) > len(corpus["alone"]["jvs001"][2][0])


def test_second_run_rewrites_nothing(corpus):
    files = [os.path.join(corpus["train"], NAMES["jvs001"]), os.path.join(corpus["train"], NAMES["p225"]),
             os.path.join(corpus["test"], NAMES["jvs002"])]
    before = [(os.stat(p).st_ino, os.stat(p).st_mtime_ns) for p in files]
    EP = _mod("embedder_preprocess")
    again = EP.EncoderPreprocessor(corpus["corpora"], corpus["train"], corpus["test"], tisv_frame=TISV,
                                   top_db=TOP_DB, batch=3, overwrite=False).save_spectrogram_tisv()
    assert dict(again) == dict(corpus["report"])
    assert [(os.stat(p).st_ino, os.stat(p).st_mtime_ns) for p in files] == before


def test_speaker_store_loads_the_result(corpus):
    ED = _mod("embedder_data")
    store = ED.SpeakerStore(corpus["train"], datasets=("JVS", "VCTK"), tisv_frame=TISV)
    assert store.files == [NAMES["jvs001"], NAMES["p225"]] and store.langs == ["en", "jp"]
    assert store.utt_count == [corpus["report"][NAMES["jvs001"]], corpus["report"][NAMES["p225"]]]
    # the batcher's variable crop length starts at tisv_frame - 0.4 s of frames, which is below
    # zero for a window of 8 frames: take whole windows
    mels, langs = ED.SpeakerBatcher(store, 2, 2, variable_length=False).next_batch()
    assert mels.shape == (4, TISV, 80) and langs.shape == (4,)
    assert torch.isfinite(mels).all()


def test_cli_writes_the_same_files(corpus):
    root, roots = corpus["root"], corpus["roots"]
    train, test = os.path.join(root, "cli_train"), os.path.join(root, "cli_test")
    cfg = os.path.join(root, "config.yaml")
    with open(cfg, "w") as f:
        f.write(f"training: !!bool \"true\"\ndatasets:\n    VCTK:\n        root: '{roots['vctk']}'\n"
                f"        test_speakers: []\n    JVS:\n        root: '{roots['jvs']}'\n"
                f"        test_speakers: ['jvs002']\ntrain_datasets: ['JVS', 'VCTK']\n---\ndata:\n"
                f"    train_path: '{train}'\n    test_path: '{test}'\n    sr: {SR}\n    nfft: 1024\n"
                f"    window: {WINDOW}\n    hop: {HOP}\n    nmels: 80\n    tisv_frame: {TISV}\n---\n"
                f"model:\n    hidden: 256\n")
    report = _mod("embedder_preprocess").main(["--config", cfg, "--top_db", str(TOP_DB),
                                               "--batch", "3"])
    assert dict(report) == dict(corpus["report"])
    for folder, new in (("train", train), ("test", test)):
        assert sorted(os.listdir(new)) == sorted(os.listdir(corpus[folder]))
        for name in os.listdir(new):
            assert np.array_equal(np.load(os.path.join(new, name)),
                                  np.load(os.path.join(corpus[folder], name)))
