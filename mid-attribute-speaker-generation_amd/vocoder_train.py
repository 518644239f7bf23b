"""Training the HiFi-GAN generator on this project's own mel front end.

Only the generator's own loss term is built: the mel-reconstruction L1 (the x45 term of
HiFi-GAN's generator loss, which as the single term needs no weight).  The MPD / MSD
discriminators and feature matching are not built; a generator trained on the mel term alone is
known to sound buzzier than a GAN-trained one, and nothing is claimed about audio quality.  What
the term does constrain is what the project's metrics read: MCD, PER and the d-vector scores all
see audio through ``audio.MelFrontEnd``, and the loss is on exactly that mel (HiFi-GAN's separate
``fmax_for_loss`` / ``center=False`` mel is deliberately not reproduced).

  MelLoss          ``melspec`` + ``mel_l1`` forward, ``melspec_bwd`` backward, one autograd node
  WaveStore        a corpus's waveforms (``corpus_io.read_wav``, ``audio.Resampler``) in one HBM
                   buffer; equal-length segments are gathered on the device (``wave_segments``)
  VocoderTrainer   ``Generator.forward_train`` + ``MelLoss`` + ``grad_norm`` / ``adam_step`` over
                   flat buffers: Adam with HiFi-GAN's betas (0.8, 0.99), lr 2e-4 decayed by 0.999
                   per epoch.  HiFi-GAN's AdamW weight decay (0.01) is dropped: ``fs2_adam_step``
                   has no decoupled decay, and with the mel term alone it only shrinks the
                   weights.  Weight norm is not re-parametrised: the folded weights move, and
                   checkpoints hold plain keys, ``{"generator": state_dict, "steps": n}``, which
                   ``hifigan.get_vocoder(ckpt=...)`` loads unchanged.

CLI: ``python -m mid-attribute-speaker-generation_amd.vocoder_train --config DIR [--corpus NAME
...] [--steps N] [--batch 16] [--segment 8192] [--checkpoint P] [--restore P] [--dtype bf16]
[--seed S]``.
"""
import argparse
import glob
import math
import os

import numpy as np
import torch
import yaml

from . import config as cfg
from . import kernels as K
from .audio import MelFrontEnd, Resampler
from .corpus_io import read_wav
from .hifigan import Generator, load_config

BETAS, LR, LR_DECAY, EPS = (0.8, 0.99), 2e-4, 0.999, 1e-8  # HiFi-GAN config_v1.json


class _MelLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wav, target, front_end):
        window, twiddle, fb = front_end._dev_tables()
        w = wav.contiguous()
        mel, _, _, _ = K.melspec(w, None, front_end.hop, window, twiddle, fb, front_end.n_mels,
                                 energy=False)
        loss, d_mel = K.mel_l1(mel, target.contiguous(), grad=True)
        ctx.front_end, ctx.wav, ctx.d_mel = front_end, w, d_mel
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        fe = ctx.front_end
        window, twiddle, fb = fe._dev_tables()
        d_wav = K.melspec_bwd(ctx.wav, None, ctx.d_mel, fe.hop, window, twiddle, fb, fe.n_mels)
        ctx.wav = ctx.d_mel = None
        return d_wav * g, None, None


class MelLoss:
    """``mean |logmel(wav) - target|`` over every element, differentiable in ``wav`` (B, S);
    ``target`` (B, n_mels, 1 + S // hop) is a log-mel of the same front end."""

    def __init__(self, front_end):
        self.front_end = front_end

    def __call__(self, wav, target):
        if wav.dim() != 2 or wav.dtype != torch.float32:
            raise ValueError("MelLoss: wav is f32 (B, S)")
        F = self.front_end.n_frames(wav.shape[1])
        if tuple(target.shape) != (wav.shape[0], self.front_end.n_mels, F):
            raise ValueError(f"MelLoss: target is (B, {self.front_end.n_mels}, {F})")
        self.front_end.check_lens([wav.shape[1]], wav.shape[1])
        return _MelLossFn.apply(wav, target, self.front_end)


class WaveStore:
    """Waveforms at the front end's rate, concatenated in one device buffer."""

    def __init__(self, waves, device="cuda"):
        """``waves``: float32 arrays / tensors already at the training rate."""
        self.device = torch.device(device)
        lens = [int(len(w)) for w in waves]
        if not lens:
            raise ValueError("WaveStore: no waveform")
        self.lens = np.asarray(lens, np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lens)[:-1]]).astype(np.int64)
        flat = torch.cat([torch.as_tensor(w, dtype=torch.float32).reshape(-1).to(self.device)
                          for w in waves])
        self.flat = flat.view(1, -1).contiguous()

    @classmethod
    def from_corpus(cls, raw_path, sr, device="cuda", batch=64):
        """Every ``raw_path/<speaker>/*.wav``, decoded on the host and resampled on the device
        (one launch per distinct file rate per ``batch`` files)."""
        paths = sorted(glob.glob(os.path.join(raw_path, "*", "*.wav")))
        if not paths:
            raise ValueError(f"no <speaker>/*.wav under {raw_path}")
        rs = Resampler(sr, device)
        waves = []
        for i in range(0, len(paths), batch):
            decoded = [read_wav(p) for p in paths[i:i + batch]]
            by_rate = {}
            for j, (x, r) in enumerate(decoded):
                by_rate.setdefault(r, []).append(j)
            out = [None] * len(decoded)
            for r, idx in by_rate.items():
                S = max(len(decoded[j][0]) for j in idx)
                host = np.zeros((len(idx), S), np.float32)
                for row, j in enumerate(idx):
                    host[row, :len(decoded[j][0])] = decoded[j][0]
                lens = [len(decoded[j][0]) for j in idx]
                y, _ = rs(torch.from_numpy(host).to(device), lens, r)
                for row, j in enumerate(idx):
                    out[j] = y[row, :rs.out_len(lens[row], r)].clone()
            waves.extend(out)
        return cls(waves, device)

    def __len__(self):
        return len(self.lens)

    def draw(self, batch, segment, generator):
        """``batch`` segments of ``segment`` samples: utterance and start by the seeded host
        ``generator``, the gather on the device.  Utterances shorter than a segment are never
        drawn (HiFi-GAN zero-pads them; ragged training batches are not built)."""
        ok = np.nonzero(self.lens >= segment)[0]
        if len(ok) == 0:
            raise ValueError(f"no utterance has {segment} samples")
        u = ok[torch.randint(len(ok), (batch,), generator=generator).numpy()]
        frac = torch.rand(batch, generator=generator, dtype=torch.float64).numpy()
        start = np.minimum((frac * (self.lens[u] - segment + 1)).astype(np.int64),
                           self.lens[u] - segment)
        return self.gather(self.offsets[u] + start, segment)

    def gather(self, first, segment):
        """Segments starting at the flat positions ``first`` (host int64)."""
        n = len(first)
        dev = self.device
        row = torch.zeros(n, dtype=torch.int32, device=dev)
        f = torch.from_numpy(np.ascontiguousarray(first, np.int64)).to(dev)
        ln = torch.full((n,), int(segment), dtype=torch.int64, device=dev)
        return K.wave_segments(self.flat, row, f, ln, int(segment))


class VocoderTrainer:
    """One training step = segments -> their own mel -> generator -> mel L1 -> Adam."""

    def __init__(self, generator, front_end, lr=LR, betas=BETAS, eps=EPS, lr_decay=LR_DECAY,
                 steps_per_epoch=None):
        self.gen, self.front_end = generator, front_end
        self.loss_fn = MelLoss(front_end)
        self.up = math.prod(generator.h.upsample_rates)
        if self.up != front_end.hop:
            raise ValueError(f"the generator upsamples by {self.up}, the front end hops {front_end.hop}")
        self.lr, self.betas, self.eps, self.lr_decay = float(lr), betas, float(eps), float(lr_decay)
        self.steps_per_epoch = steps_per_epoch
        self.steps = 0
        params = list(generator.parameters())
        dev = params[0].device
        n = sum(p.numel() for p in params)
        # flat fp32 masters, gradients and moments: the parameters become views of `flat`
        self.flat = torch.empty(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.m, self.v = torch.zeros_like(self.grad), torch.zeros_like(self.grad)
        off = 0
        with torch.no_grad():
            for p in params:
                view = self.flat[off:off + p.numel()].view(p.shape)
                view.copy_(p)
                p.data = view
                p.requires_grad_(True)
                p.grad = self.grad[off:off + p.numel()].view(p.shape)
                off += p.numel()
        generator.weights_changed()
        self.norm_coef = torch.zeros(2, dtype=torch.float32, device=dev)

    def current_lr(self):
        epoch = self.steps // self.steps_per_epoch if self.steps_per_epoch else 0
        return self.lr * self.lr_decay ** epoch

    def step(self, segments):
        """segments (B, S) f32 on the device, S a multiple of the hop -> (mel loss, gradient
        norm), both 0-dim device tensors."""
        B, S = segments.shape
        if S % self.up:
            raise ValueError(f"segment {S} is not a multiple of the hop {self.up}")
        T = S // self.up
        with torch.no_grad():
            target = self.front_end(segments)[0]                       # (B, n_mels, T + 1)
            rows = target[:, :, :T].transpose(1, 2).contiguous().view(B * T, -1)
        K.fill_(self.grad, 0.0)
        wav = self.gen.forward_train(rows, B, T)
        loss = self.loss_fn(wav.view(B, S), target)
        loss.backward()
        K.grad_norm(self.grad, 1e30, self.norm_coef)  # no clipping: the norm is only logged
        self.steps += 1
        b1, b2 = self.betas
        K.adam_step(self.flat, self.grad, self.m, self.v, self.norm_coef, self.current_lr(), b1, b2,
                    self.eps, 1.0 - b1 ** self.steps, math.sqrt(1.0 - b2 ** self.steps))
        self.gen.weights_changed()
        return loss.detach(), self.norm_coef[0]

    # ------------------------------------------------------------ checkpoints
    def state_dict(self):
        return {"generator": {k: v.detach().clone() for k, v in self.gen.state_dict().items()},
                "steps": self.steps, "m": self.m.clone(), "v": self.v.clone()}

    def save(self, path):
        torch.save(self.state_dict(), path)

    def restore(self, path):
        sd = torch.load(path, map_location=self.flat.device, weights_only=True)
        self.gen.load_state_dict(sd["generator"])
        self.steps = int(sd.get("steps", 0))
        if "m" in sd and sd["m"].numel() == self.m.numel():
            self.m.copy_(sd["m"])
            self.v.copy_(sd["v"])
        self.gen.weights_changed()


def fit(trainer, store, steps, batch, segment, seed=0, log_step=100, save_step=None,
        checkpoint=None, log=print):
    gen = torch.Generator().manual_seed(int(seed) + trainer.steps)
    trainer.steps_per_epoch = trainer.steps_per_epoch or max(1, -(-len(store) // batch))
    while trainer.steps < steps:
        loss, gnorm = trainer.step(store.draw(batch, segment, gen))
        if trainer.steps % log_step == 0 or trainer.steps == steps:
            log(f"Step {trainer.steps}/{steps}, Mel Loss: {float(loss):.4f}, "
                f"Grad Norm: {float(gnorm):.3f}, lr: {trainer.current_lr():.3e}")
        if checkpoint and save_step and trainer.steps % save_step == 0:
            trainer.save(checkpoint)
    if checkpoint:
        trainer.save(checkpoint)
    return trainer.steps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("-c", "--config", type=str, required=True, help="path to config")
    ap.add_argument("--corpus", nargs="*", type=str, default=None)
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--segment", type=int, default=8192)
    ap.add_argument("--checkpoint", type=str, default=None, help="where to save")
    ap.add_argument("--restore", type=str, default=None, help="a checkpoint to continue from")
    ap.add_argument("--dtype", choices=("fp32", "bf16"), default="bf16")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--vocoder_config", type=str, default=None, help="hifigan.json (bundled)")
    args = ap.parse_args(argv)

    pp, _, tc, path = cfg.load_configs(args.config)
    if args.corpus is not None:
        files = [os.path.join(path, f"preprocess_{c}.yaml") for c in args.corpus]
    else:
        files = sorted(glob.glob(os.path.join(path, "preprocess_*.yaml")))
    if not files:
        raise ValueError(f"no preprocess_<corpus>.yaml under {path}")
    front_end = MelFrontEnd(pp, device="cuda")
    waves = []
    for f in files:
        with open(f) as fh:
            raw = yaml.safe_load(fh)["path"]["raw_path"]
        waves.append(WaveStore.from_corpus(raw, front_end.sr, "cuda"))
    store = waves[0] if len(waves) == 1 else WaveStore(
        [w.flat[0, o:o + n] for w in waves for o, n in zip(w.offsets, w.lens)], "cuda")
    from .seeded import load_seeded_
    gen = Generator(load_config(args.vocoder_config), device="cuda",
                    compute_dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32)
    load_seeded_(gen)
    trainer = VocoderTrainer(gen, front_end)
    if args.restore:
        trainer.restore(args.restore)
    step_cfg = tc.get("step", {})
    print("Number of generator parameters:", trainer.flat.numel())
    last = fit(trainer, store, args.steps, args.batch, args.segment, seed=args.seed,
               log_step=int(step_cfg.get("log_step", 100)),
               save_step=int(step_cfg.get("save_step", 0)) or None, checkpoint=args.checkpoint)
    print(f"finished at step {last}")


if __name__ == "__main__":
    main()
