"""Are the generated speakers any good: set-to-set statistics in speaker-encoder space.

A speaker drawn from an attribute prior has no recording, so ``metrics`` (MCD, F0, ``DVEC_COS``
against a ground truth) cannot score it.  What can be measured, in the spirit of TacoSpawn's
speaker-distance tables, is where the generated voices lie relative to the training voices:

* ``g2t`` against ``t2t``: is a generated speaker as far from its nearest training speaker as
  training speakers are from each other (novel), or far closer (memorised);
* ``g2g`` against ``t2t``: are generated speakers as far from one another as real ones (diverse);
* ``g_within`` against ``t_within``: does one generated voice stay itself across texts (stable);
* ``fd_g_t`` against the floor ``fd_t_t``: does the generated cloud have the distribution of the
  real one (Frechet distance of the Gaussians fitted to the utterance d-vectors);
* ``attribute_vote``: does an interpolation at rate t land between the two attribute groups.

All distances are cosine distances between unit-length d-vectors (or speaker centroids) of THIS
project's speaker encoder: they compare runs that share an encoder checkpoint and nothing else.

The arithmetic is ``csrc/speaker_eval.hip`` (``kernels.cosine_nn``, ``finite_summary``,
``gauss_moments``, ``frechet``); this module is the bookkeeping, written against a small set of
operations (``nearest``, ``summary``, ``centroids``, ``frechet``) so that ``table`` runs on any
implementation of them -- the tests run it on a numpy oracle without the library.
"""
import json
import os

import torch

from . import kernels as K


# ------------------------------------------------------------------ device operations
def nearest(a, b, k=1, group_a=None, group_b=None, same=False):
    """``(dist (Na, k), index (Na, k))``: the k rows of b nearest to each row of a by cosine
    distance (``kernels.cosine_nn``); candidates of the row's own group are skipped, or with
    ``same`` the only ones kept."""
    return K.cosine_nn(a.detach().float().contiguous(), b.detach().float().contiguous(), k,
                       group_a, group_b, same)


FIELDS = ("count", "median", "mean", "min", "max")


def summary(x):
    """``{count, median, mean, min, max}`` of the finite entries of x; one host read."""
    r = K.finite_summary(x.detach().float().contiguous().view(-1)).tolist()
    return {"count": int(r[0]), **dict(zip(FIELDS[1:], r[1:]))}


def _seg_tensor(seg_start, device):
    if torch.is_tensor(seg_start):
        return seg_start.to(device=device, dtype=torch.int64).contiguous()
    return torch.tensor([int(s) for s in seg_start], dtype=torch.int64).to(device)


def centroids(dvecs, seg_start):
    """Per-speaker unit-length mean d-vectors (``kernels.rows_mean_unit``); rows are grouped by
    speaker, speaker s owning rows seg_start[s] .. seg_start[s + 1] - 1."""
    x = dvecs.detach().float().contiguous()
    return K.rows_mean_unit(x, _seg_tensor(seg_start, x.device))


def frechet(a, b):
    """Frechet distance of the Gaussians fitted to the rows of a and of b (each at least 2 rows,
    width at most 64); one host read."""
    ma, ca = K.gauss_moments(a.detach().float().contiguous())
    mb, cb = K.gauss_moments(b.detach().float().contiguous())
    return K.frechet(ma, ca, mb, cb)[0, 0].item()


def attribute_vote(points, ref_points, ref_labels, k=5):
    """Per point, the fraction of its k nearest reference speakers that carry label 1 (device
    tensor (N) f32; NaN for a point without neighbours)."""
    _, idx = nearest(points, ref_points, min(int(k), K.NN_MAX_K))
    labels = torch.as_tensor(ref_labels).to(idx.device).long()
    found = idx >= 0
    ones = (labels[idx.clamp_min(0)] == 1) & found
    return ones.sum(1).float() / found.sum(1).float()


# ------------------------------------------------------------------ the table
class SpeakerSet:
    """Utterance d-vectors (N, D), rows grouped by speaker, and ``seg_start`` (host ints,
    n_speakers + 1): speaker s owns rows seg_start[s] .. seg_start[s + 1] - 1."""

    def __init__(self, dvecs, seg_start):
        self.dvecs = dvecs
        self.seg_start = [int(s) for s in (seg_start.tolist() if torch.is_tensor(seg_start)
                                           else seg_start)]
        if self.seg_start[0] != 0 or self.seg_start[-1] != dvecs.shape[0] or \
                any(b <= a for a, b in zip(self.seg_start[:-1], self.seg_start[1:])):
            raise ValueError(f"seg_start {self.seg_start} does not cut {dvecs.shape[0]} rows into "
                             "non-empty speakers")

    @property
    def n_speakers(self):
        return len(self.seg_start) - 1

    def speaker_of_row(self):
        """(N) int64 on the d-vectors' device: the speaker index of every row."""
        ids = [s for s in range(self.n_speakers)
               for _ in range(self.seg_start[s + 1] - self.seg_start[s])]
        return torch.tensor(ids, dtype=torch.int64).to(self.dvecs.device)

    def rows_of(self, speakers):
        """The d-vectors of the listed speakers, in that order."""
        parts = [self.dvecs[self.seg_start[s]:self.seg_start[s + 1]] for s in speakers]
        return torch.cat(parts) if parts else self.dvecs[:0]


class _DeviceOps:
    """The four operations ``table`` is written against, on the kernels."""
    nearest = staticmethod(nearest)
    summary = staticmethod(summary)
    centroids = staticmethod(centroids)
    frechet = staticmethod(frechet)


def _index(n, like):
    return torch.arange(n, dtype=torch.int64).to(like.device)


def _others(ops, c):
    """Each row's distance to its nearest OTHER row of the same set."""
    idx = _index(c.shape[0], c)
    return ops.summary(ops.nearest(c, c, 1, idx, idx)[0])


def _fd(ops, a, b):
    return ops.frechet(a, b) if a.shape[0] >= 2 and b.shape[0] >= 2 else float("nan")


def table(ops, train, generated, truth=None):
    """``distance_table`` on the operations of ``ops`` (this module's, or an oracle's)."""
    ct, cg = ops.centroids(train.dvecs, train.seg_start), ops.centroids(generated.dvecs,
                                                                        generated.seg_start)
    out = {"t2t": _others(ops, ct), "g2g": _others(ops, cg),
           "g2t": ops.summary(ops.nearest(cg, ct, 1)[0]),
           "t2g": ops.summary(ops.nearest(ct, cg, 1)[0])}
    for name, s, c in (("t_within", train, ct), ("g_within", generated, cg)):
        d, _ = ops.nearest(s.dvecs, c, 1, s.speaker_of_row(), _index(s.n_speakers, c), same=True)
        out[name] = ops.summary(d)
    out["fd_g_t"] = _fd(ops, generated.dvecs, train.dvecs)
    out["fd_t_t"] = _fd(ops, train.rows_of(range(0, train.n_speakers, 2)),
                        train.rows_of(range(1, train.n_speakers, 2)))
    if truth is not None:
        if truth.n_speakers != train.n_speakers:
            raise ValueError(f"truth has {truth.n_speakers} speakers, train {train.n_speakers}: "
                             "they are the same speakers in the same order")
        cs = ops.centroids(truth.dvecs, truth.seg_start)
        idx = _index(cs.shape[0], cs)
        out["s2s"] = _others(ops, cs)
        out["s2t"] = ops.summary(ops.nearest(cs, ct, 1)[0])
        out["s2t_same"] = ops.summary(ops.nearest(cs, ct, 1, idx, idx, same=True)[0])
    return out


def distance_table(train, generated, truth=None):
    """The speaker-distance table of two ``SpeakerSet`` s (synthesised training speakers and
    generated speakers), every entry a ``summary`` record of cosine distances:

    * speaker level, between centroids: ``t2t`` each training speaker to its nearest other
      training speaker, ``g2g`` the same among generated speakers, ``g2t`` each generated speaker
      to its nearest training speaker, ``t2g`` each training speaker to its nearest generated one;
    * utterance level: ``t_within`` / ``g_within`` each utterance to its own speaker's centroid;
    * distribution level (floats): ``fd_g_t`` the Frechet distance between all generated and all
      training utterance d-vectors, ``fd_t_t`` between the training speakers at even and at odd
      positions, the noise floor (NaN when a side has fewer than 2 rows);
    * with ``truth``, d-vectors of recordings of the training speakers in the same order (from
      ``EmbedderTrainer.dvector_from_wav``, say): ``s2s`` recorded speakers among themselves,
      ``s2t`` each to its nearest synthesised training speaker, ``s2t_same`` each to its own.

    Novel: the ``g2t`` median near the ``t2t`` median, memorised when far below.  Diverse:
    ``g2g`` near ``t2t``.  Stable: ``g_within`` near ``t_within``."""
    return table(_DeviceOps, train, generated, truth)


# ------------------------------------------------------------------ drawing and synthesis
def draw(prior, n, seed=0):
    """n embeddings (n, d) from the first row of a ``GMMPrior``; row 0 is what
    ``prior.sample(seed=seed)`` / ``speaker_gen(seed=seed)`` draws."""
    k, d = prior.pi.shape[-1], prior.mu.shape[-1]
    pi = prior.pi.reshape(-1, k)[:1].expand(n, k).contiguous()
    mu = prior.mu.reshape(-1, k, d)[:1].expand(n, k, d).contiguous()
    sd = prior.sigma.reshape(-1, k, d)[:1].expand(n, k, d).contiguous()
    return K.gmm_sample(pi, mu, sd, int(seed), 0)[0]


def embedding_space_report(model, priors, n, seed=0):
    """``{prior name: {t2t, g2g, g2t}}`` in the model's own speaker-embedding space: the rows of
    the speaker table against n samples of each prior.  No synthesis."""
    rows = model.speaker_emb.weight.detach().float().contiguous()
    t2t = _others(_DeviceOps, rows)
    out = {}
    for name, prior in priors.items():
        g = draw(prior, n, seed)
        out[name] = {"t2t": t2t, "g2g": _others(_DeviceOps, g),
                     "g2t": summary(nearest(g, rows, 1)[0])}
    return out


def _text_fields(batch):
    if len(batch) not in (8, 14):
        raise ValueError(f"a text batch is the 8-tuple synth_dvectors takes or the 14-tuple of a "
                         f"CorpusBatcher with accents, got {len(batch)} fields")
    return batch[3], batch[4], batch[5], batch[-1]


@torch.no_grad()
def synth_speaker_set(model, vocoder, trainer, batches, embs, control_values=(1.0, 1.0, 1.0),
                      hop_length=256, recognizer=None):
    """Every text batch in the voice of every row of ``embs`` (S, d) -> ``SpeakerSet`` of the
    utterances' d-vectors, speaker-major.  The embedding goes in per batch row, (B, d).  With
    ``recognizer`` (a ``recognizer.RecognizerTrainer``) the result is ``(SpeakerSet, sums)``:
    the device int64 sums ``metrics.PER_FIELDS`` of ``metrics.phoneme_error_rate`` of every
    synthesised mel (``out[1]``, ``out[9]`` frames) against its text."""
    from .synthesize import output_dvectors
    per_sums = None
    if recognizer is not None:
        from . import metrics
        per_sums = torch.zeros(len(metrics.PER_FIELDS), dtype=torch.int64, device=embs.device)
    p_c, e_c, d_c = control_values
    was = model.training
    model.eval()
    dvecs, seg = [], [0]
    try:
        for s in range(embs.shape[0]):
            n = 0
            for batch in batches:
                texts, src_lens, max_src_len, accents = _text_fields(batch)
                emb = embs[s:s + 1].expand(texts.shape[0], -1).contiguous()
                out = model.synthesize_from_speaker_emb(
                    None, texts, src_lens, max_src_len, p_control=p_c, e_control=e_c,
                    d_control=d_c, accents=accents, speaker_emb=emb)
                dvecs.append(output_dvectors(out, vocoder, trainer, hop_length))
                if recognizer is not None:
                    post = out[1].contiguous()
                    per_sums += metrics.phoneme_error_rate(
                        recognizer, post, out[9].clamp(1, post.shape[1]), texts, src_lens)
                n += texts.shape[0]
            seg.append(seg[-1] + n)
    finally:
        model.train(was)
    out = SpeakerSet(torch.cat(dvecs).contiguous(), seg)
    return out if recognizer is None else (out, per_sums)


def speaker_labels(config_path, metadata, attribute):
    """Per speaker id, the index of its ``attribute`` value: ``speakers.json`` maps a name to
    ``[id, value of metadata attribute 0, value of attribute 1, ...]``, ``metadata`` is the
    ``speaker_generation.metadata`` section (attribute -> {value: index})."""
    with open(os.path.join(config_path, "speakers.json")) as f:
        speakers = json.load(f)
    pos = list(metadata).index(attribute)
    labels = [None] * len(speakers)
    for name, entry in speakers.items():
        if not isinstance(entry, (list, tuple)) or len(entry) <= pos + 1:
            raise ValueError(f"speakers.json gives no metadata for {name}: a preprocessed "
                             "corpus's file lists [id, values...] per speaker")
        labels[int(entry[0])] = int(metadata[attribute][entry[pos + 1]])
    return labels


def evaluate_generated(model, vocoder, trainer, batches, priors, n_speakers, train_speakers=None,
                       attribute=None, seed=0, control_values=(1.0, 1.0, 1.0), hop_length=256,
                       config_path=None, recognizer=None):
    """The full evaluation: for each named prior (a ``GMMPrior`` from ``speaker_distribution``,
    an ``InterpolateGMM`` at a rate, a ``BarycenterGMM``) draw ``n_speakers`` embeddings
    (``draw``), synthesise every text batch for each of them and for the training speakers
    ``train_speakers`` (speaker-table rows; default all) with ``vocoder`` (anything with
    ``forward_rows``), take the utterances' d-vectors with ``trainer`` and build the
    ``distance_table``.  ``batches`` is a list of device text batches.

    Returns ``{"tables": {prior: table}, "sets": {"train": SpeakerSet, prior: SpeakerSet}}``; with
    ``attribute`` -- per training speaker of ``train_speakers`` a 0/1 label, or an attribute name
    looked up by ``speaker_labels`` in ``config_path``'s speakers.json -- also ``"vote": {prior: mean
    attribute_vote of the generated speakers' centroids against the training speakers'}``.

    With ``recognizer`` (a ``recognizer.RecognizerTrainer``; default None: the keys are those
    above) also ``"per": {"train": ..., prior: ...}``, per set the phoneme error rate of its
    synthesised mels against the texts (``metrics.phoneme_error_rate`` on the PostNet mel, no
    vocoder involved; one host read per set): whether a voice drawn from the prior still speaks
    the text.  The figures are those of this recogniser checkpoint; see ``metrics``."""
    batches = list(batches)
    table_rows = model.speaker_emb.weight.detach().float()
    ids = list(range(table_rows.shape[0])) if train_speakers is None else \
        [int(s) for s in train_speakers]
    kw = dict(control_values=control_values, hop_length=hop_length)
    per = {}

    def synth(name, embs):
        if recognizer is None:
            return synth_speaker_set(model, vocoder, trainer, batches, embs, **kw)
        from . import metrics
        out, sums = synth_speaker_set(model, vocoder, trainer, batches, embs,
                                      recognizer=recognizer, **kw)
        per[name] = metrics.per_from_sums(sums.tolist())["per"]
        return out

    train = synth("train", table_rows[torch.tensor(ids).to(table_rows.device)].contiguous())
    labels = None
    if isinstance(attribute, str):
        if config_path is None:
            raise ValueError("an attribute name needs config_path, the directory of speakers.json")
        every = speaker_labels(config_path, model.speaker_enc.metadata_list, attribute)
        labels = [every[s] for s in ids]
    elif attribute is not None:
        labels = [int(v) for v in attribute]
        if len(labels) != len(ids):
            raise ValueError(f"{len(labels)} attribute labels for {len(ids)} training speakers")
    out = {"tables": {}, "sets": {"train": train}}
    if labels is not None:
        out["vote"] = {}
        ct = centroids(train.dvecs, train.seg_start)
    for name, prior in priors.items():
        gen = synth(name, draw(prior, n_speakers, seed))
        out["sets"][name] = gen
        out["tables"][name] = distance_table(train, gen)
        if labels is not None:
            votes = attribute_vote(centroids(gen.dvecs, gen.seg_start), ct, labels)
            out["vote"][name] = summary(votes)["mean"]
    if recognizer is not None:
        out["per"] = per
    return out


# ------------------------------------------------------------------ command line
def _one_hot_meta(metadata, attribute, value_index, device):
    """The metadata one-hot with ``attribute`` at ``value_index`` and every other attribute at
    its first value."""
    v = []
    for name, values in metadata.items():
        hot = value_index if name == attribute else 0
        v += [1.0 if i == hot else 0.0 for i in range(len(values))]
    return torch.tensor([v], dtype=torch.float32).to(device)


def _jsonable(x):
    """NaN and the infinities have no JSON form: they become null."""
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, float) and x - x != 0.0:
        return None
    return x


def main(argv=None):
    """``python -m mid-attribute-speaker-generation_amd.speaker_eval -c DIR --restore_step N
    --embedder CKPT [--checkpoint P] [--corpus NAME ...] [--vocoder hifigan|griffinlim]
    [--n_speakers 100] [--n_texts 20] [--attribute gender --rates 0 0.25 0.5 0.75 1] [--seed S]
    [--recognizer CKPT] [--out report.json]``

    ``DIR`` is a training config directory (as ``train`` takes).  Texts are the first
    ``n_texts`` utterances of the validation list.  Without ``--rates`` the priors are the
    attribute's two values; with them, ``InterpolateGMM`` between the two at those rates.  The
    report is one JSON object: per prior its table, and with ``--attribute`` the vote (the share
    of a generated speaker's 5 nearest training speakers that carry the attribute's second
    value) and the ``g2t`` median per rate; with ``--recognizer`` (a checkpoint of
    ``recognize``) ``per``, the phoneme error rate of the training speakers' and of each prior's
    synthesised mels."""
    import argparse
    import glob

    import yaml

    from . import config as cfg
    from .corpus_store import CorpusBatcher, CorpusStore
    from .dataset import ConcatDataset, Dataset, corpus_config
    from .distributions import InterpolateGMM
    from .embedder_train import EmbedderTrainer
    from .loss import feature_levels
    from .model import FastSpeech2

    ap = argparse.ArgumentParser(prog="python -m mid-attribute-speaker-generation_amd.speaker_eval")
    ap.add_argument("-c", "--config", type=str, required=True)
    ap.add_argument("--restore_step", type=int, default=0)
    ap.add_argument("--checkpoint", type=str, help="FastSpeech2 weights, instead of --restore_step")
    ap.add_argument("--embedder", type=str, required=True, help="speaker-encoder checkpoint")
    ap.add_argument("--corpus", nargs="*", type=str, default=None,
                    help="the corpora to read val.txt from, in order (default: all, sorted)")
    ap.add_argument("--vocoder", choices=("hifigan", "griffinlim"), default="griffinlim")
    ap.add_argument("--n_speakers", type=int, default=100)
    ap.add_argument("--n_texts", type=int, default=20)
    ap.add_argument("--attribute", type=str, default=None)
    ap.add_argument("--rates", type=float, nargs="*", default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--recognizer", type=str, default=None,
                    help="a recogniser checkpoint (recognize): add the phoneme error rate of "
                         "every set's synthesised mels to the report")
    args = ap.parse_args(argv)
    if args.recognizer is not None and not os.path.isfile(args.recognizer):
        ap.error(f"--recognizer {args.recognizer}: no such file")

    pp, mc, tc, path = cfg.load_configs(args.config)
    model = FastSpeech2(pp, mc, path, device="cuda")
    ckpt = args.checkpoint or os.path.join(tc["path"]["ckpt_path"], f"{args.restore_step}.pth.tar")
    model.load_state_dict(torch.load(ckpt, map_location="cuda", weights_only=True)["model"])
    model.eval()
    trainer = EmbedderTrainer(device="cuda")
    trainer.load_state_dict(torch.load(args.embedder, map_location="cuda", weights_only=True))
    if args.vocoder == "hifigan":
        from .hifigan import get_vocoder
        vocoder = get_vocoder(device="cuda", ckpt=tc["path"].get("vocoder_path"))
    else:
        from .audio import GriffinLim
        vocoder = GriffinLim(pp)
        vocoder.generator = torch.Generator(device="cuda").manual_seed(args.seed)

    if args.corpus is not None:
        files = [os.path.join(path, f"preprocess_{c}.yaml") for c in args.corpus]
    else:
        files = sorted(glob.glob(os.path.join(path, "preprocess_*.yaml")))
    corpora = []
    for f in files:
        with open(f) as fh:
            corpora.append(yaml.safe_load(fh))
    if not corpora:
        raise ValueError(f"no preprocess_<corpus>.yaml under {path}")
    sets = [Dataset("val.txt", corpus_config(pp, c), tc) for c in corpora]
    store = CorpusStore(ConcatDataset(path, sets), device="cuda", levels=feature_levels(pp))
    n_texts = min(args.n_texts, len(store))
    bs = max(d for d in range(1, tc["optimizer"]["batch_size"] + 1) if n_texts % d == 0)
    batches = []
    for batch in CorpusBatcher(store, bs, group_size=1, shuffle=False, sort=False, drop_last=False):
        if len(batches) * bs >= n_texts:
            break
        batches.append(batch)

    metadata = model.speaker_enc.metadata_list
    attribute = args.attribute or next(iter(metadata))
    if len(metadata[attribute]) != 2:
        raise ValueError(f"attribute {attribute} has {len(metadata[attribute])} values; the "
                         "interpolation runs between two")
    ends = [model.speaker_distribution(_one_hot_meta(metadata, attribute, i, "cuda"))
            for i in range(2)]
    if args.rates:
        priors = {}
        for t in args.rates:
            g = InterpolateGMM(ends[0], ends[1])
            g.interpolate_rate(float(t))
            priors[f"{attribute}@{t:g}"] = g
    else:
        priors = dict(zip(metadata[attribute], ends))
    recognizer = None
    if args.recognizer is not None:
        from .recognizer import load_recognizer
        recognizer = load_recognizer(args.recognizer, "cuda")
    res = evaluate_generated(model, vocoder, trainer, batches, priors, args.n_speakers,
                             attribute=args.attribute, seed=args.seed,
                             hop_length=pp["stft"]["hop_length"], config_path=path,
                             recognizer=recognizer)
    report = {"tables": res["tables"],
              "embedding_space": embedding_space_report(model, priors, args.n_speakers, args.seed),
              "g2t_median": {k: v["g2t"]["median"] for k, v in res["tables"].items()}}
    if "vote" in res:
        report["vote"] = res["vote"]
    if "per" in res:
        report["per"] = res["per"]
    text = json.dumps(_jsonable(report), indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return report


if __name__ == "__main__":
    main()
