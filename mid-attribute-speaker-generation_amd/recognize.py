"""Train the phoneme recogniser behind the phoneme error rate (``recognizer.py``):

    python -m mid-attribute-speaker-generation_amd.recognize --config DIR [--corpus NAME ...]
        [--steps N] [--batch B] [--checkpoint P] [--seed S]

``DIR`` is a training config directory as ``train`` takes.  The ``train.txt`` utterances of the
corpora are put on the device by ``CorpusStore`` and batched by ``CorpusBatcher``; of each batch
tuple the texts, src_lens, mels and mel_lens are used.  After ``--steps`` updates the PER on
``val.txt`` is printed and the checkpoint written to ``--checkpoint`` (default
``<ckpt_path>/recognizer.pt``), the file ``train --synth_recognizer`` and ``speaker_eval
--recognizer`` load.
"""
import os

import torch

from .recognizer import PhonemeRecognizer, RecognizerTrainer


def batch_fields(batch):
    """(texts, src_lens, mels, mel_lens) of a ``CorpusStore`` batch tuple, lengths as int64."""
    return (batch[3].contiguous(), batch[4].long().contiguous(), batch[6].contiguous(),
            batch[7].long().contiguous())


def train_recognizer(train_batcher, val_batcher, n_symbols, n_mels, steps, seed=0, lr=1e-3,
                     device="cuda", **shape):
    """``steps`` updates over the epochs of ``train_batcher`` -> ``(trainer, validation PER)``."""
    from . import metrics
    torch.manual_seed(int(seed))
    trainer = RecognizerTrainer(PhonemeRecognizer(n_symbols, n_mels, device=device, **shape), lr)

    def epochs():
        while True:
            n = 0
            for batch in train_batcher:
                n += 1
                yield batch_fields(batch)
            if n == 0:
                raise ValueError("recognize: the training corpus yields no batch")

    trainer.fit(epochs(), int(steps))
    sums = torch.zeros(5, dtype=torch.int64, device=device)
    for batch in val_batcher:
        texts, src_lens, mels, mel_lens = batch_fields(batch)
        sums += metrics.phoneme_error_rate(trainer, mels, mel_lens, texts, src_lens)
    return trainer, metrics.per_from_sums(sums.tolist())  # the pass's one host read


def main(argv=None):
    import argparse
    import glob

    import yaml

    ap = argparse.ArgumentParser(prog="python -m mid-attribute-speaker-generation_amd.recognize")
    ap.add_argument("-c", "--config", type=str, required=True, help="path to config")
    ap.add_argument("--corpus", nargs="*", type=str, default=None,
                    help="set name of corpus if only use some corpuses")
    ap.add_argument("--steps", type=int, default=20000, help="recogniser updates")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--checkpoint", type=str, default=None,
                    help="where the trained recogniser goes (default <ckpt_path>/recognizer.pt)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.steps < 1 or args.batch < 1:
        ap.error(f"--steps {args.steps} and --batch {args.batch} are at least 1")
    from . import config as cfg
    if not os.path.isdir(cfg.config_dir(args.config)):
        ap.error(f"--config {args.config}: no such directory")

    from .corpus_store import CorpusBatcher, CorpusStore
    from .dataset import ConcatDataset, Dataset, corpus_config, symbol_table
    from .loss import feature_levels

    pp, mc, tc, path = cfg.load_configs(args.config)
    if args.corpus is not None:
        files = [os.path.join(path, f"preprocess_{c}.yaml") for c in args.corpus]
    else:
        files = sorted(glob.glob(os.path.join(path, "preprocess_*.yaml")))
    if not files:
        raise ValueError(f"no preprocess_<corpus>.yaml under {path}")
    corpora = []
    for f in files:
        with open(f) as fh:
            corpora.append(yaml.safe_load(fh))
    levels = feature_levels(pp)

    def store(filename):
        sets = [Dataset(filename, corpus_config(pp, c), tc, sort=False, drop_last=False)
                for c in corpora]
        return CorpusStore(ConcatDataset(path, sets), device="cuda", levels=levels)

    gen = torch.Generator().manual_seed(int(args.seed))
    train_batcher = CorpusBatcher(store("train.txt"), args.batch, group_size=1, shuffle=True,
                                  sort=False, drop_last=False, generator=gen)
    val_batcher = CorpusBatcher(store("val.txt"), args.batch, group_size=1, shuffle=False,
                                sort=False, drop_last=False)
    trainer, figures = train_recognizer(train_batcher, val_batcher, len(symbol_table()),
                                        pp["mel"]["n_mel_channels"], args.steps, args.seed)
    out = args.checkpoint or os.path.join(tc["path"]["ckpt_path"], "recognizer.pt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    trainer.save(out)
    print("recognize: {} steps, validation PER {:.2%} ({} errors / {} phonemes: {} substitutions, "
          "{} deletions, {} insertions) -> {}".format(
              trainer.step, figures["per"], figures["distance"], figures["phonemes"],
              figures["substitutions"], figures["deletions"], figures["insertions"], out))
    return figures, out


if __name__ == "__main__":
    main()
