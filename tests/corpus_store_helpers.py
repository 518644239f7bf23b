"""Corpora for the corpus-store tests: ``synth_corpus.make_corpora`` (13 JA + 11 EN utterances)
plus what that maker does not write -- a ``val.txt``, frame-level features, fp64 energies."""
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from synth_corpus import make_corpora  # noqa: E402

D = importlib.import_module("mid-attribute-speaker-generation_amd.dataset")


def corpora_at(root, seed=0):
    """``make_corpora`` under ``root`` -> ``(config_dir, [JA, EN], preprocess, train_config)``."""
    os.makedirs(root, exist_ok=True)
    return make_corpora(root, seed=seed)


def datasets(corpus, order=(0, 1), sort=True, drop_last=True, filename="train.txt"):
    """The ``ConcatDataset`` of the corpora in ``order`` (0 = JA, with accents; 1 = EN)."""
    cfg_dir, corpora, pp, tc = corpus
    sets = [D.Dataset(filename, D.corpus_config(pp, corpora[k]), tc, sort=sort, drop_last=drop_last)
            for k in order]
    return D.ConcatDataset(cfg_dir, sets)


def _lines(pre, filename="train.txt"):
    with open(os.path.join(pre, filename), encoding="utf-8") as f:
        return [l for l in f.read().split("\n") if l]


def set_level(corpus, key, level, only=(0, 1), dtype=None, seed=7):
    """Rewrite feature ``key`` (``pitch`` / ``energy``) of the corpora ``only`` with one value per
    phoneme (``phoneme_level``) or per mel frame (``frame_level``), in ``dtype`` (default: the
    dtype on disk), drawn in the maker's value ranges."""
    rng = np.random.default_rng(seed)
    lo, hi = (80, 400) if key == "pitch" else (0, 80)
    for k in only:
        pre = corpus[1][k]["path"]["preprocessed_path"]
        for line in _lines(pre):
            base, spk = line.split("|")[:2]
            dur = np.load(os.path.join(pre, "duration", f"{spk}-duration-{base}.npy"))
            path = os.path.join(pre, key, f"{spk}-{key}-{base}.npy")
            n = int(dur.sum()) if level == "frame_level" else len(dur)
            np.save(path, rng.uniform(lo, hi, size=n).astype(dtype or np.load(path).dtype))


def write_val(corpus, n_ja=7, n_en=6):
    """``val.txt``: the first ``n_ja`` / ``n_en`` lines of each corpus's ``train.txt``."""
    for k, n in enumerate((n_ja, n_en)):
        pre = corpus[1][k]["path"]["preprocessed_path"]
        with open(os.path.join(pre, "val.txt"), "w", encoding="utf-8") as f:
            f.write("\n".join(_lines(pre)[:n]) + "\n")
