"""Captures the frame-level pitch / energy fixtures from the *reference itself* (CPU, fp32,
dropout off, name-seeded weights), the way ``oracle/make_golden.py`` captures g5 / g6.  Run in
the build container (``python scripts/make_golden_frame_level.py``); no test calls it and only
data leaves it.  Frame-level configs are the bundled JVS-VCTK dicts, deep-copied, with
``pitch.feature`` / ``energy.feature`` changed.

  g12_frame_step_b3_t16.npz   g5's recipe and keys (3 training steps at B = 3, Ts = 16) with both
                              features frame-level.  ``pred_probe`` stacks the (B, Ts)
                              predictions (here log_d only), ``frame_pred_probe`` the (B, T_mel)
                              ones (pitch, energy), in the order pitch, energy, log_d.
  g12_mixed_step_b3_t16.npz   the same with pitch phoneme-level and energy frame-level
  g13_frame_infer.npz         eval mode like g6, both frame-level: (A) no targets, p_control and
                              d_control != 1; (B) teacher-forced forward + the six losses

The batch (``data.syn_batch_for(..., pitch_level=, energy_level=)``) is checked to have an
utterance ending exactly at max_mel_len, one at least 9 frames short of it, and a zero duration.
"""
import copy
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import make_golden as mg  # noqa: E402

PKG, OUT = mg.PKG, mg.OUT
SEED = 0


def configs(levels):
    pp, mc, tc, path = PKG.config.load_configs("JVS-VCTK")
    pp, mc, tc = copy.deepcopy(pp), copy.deepcopy(mc), copy.deepcopy(tc)
    pp["pitch"]["feature"], pp["energy"]["feature"] = levels
    return pp, mc, tc, path


def batch_for(B, Ts, levels, seed=SEED):
    b = PKG.data.syn_batch_for("JVS-VCTK", B, Ts, seed=seed, pitch_level=levels[0],
                               energy_level=levels[1])
    mel_lens, Tm, src_lens, dur = b[7], b[8], b[4], b[11]
    assert (mel_lens == Tm).any(), "no utterance ends at max_mel_len"
    assert (mel_lens <= Tm - 9).any(), "no utterance ends 9 frames short of max_mel_len"
    assert any((dur[i, :src_lens[i]] == 0).any() for i in range(B)), "no zero duration"
    for i, lv in ((9, levels[0]), (10, levels[1])):
        assert b[i].shape == ((B, Tm) if lv == "frame_level" else (B, Ts))
    return PKG.data.to_device(b, "cpu")


def g12(fs2, loss_mod, levels, name, B=3, Ts=16, steps=3):
    from model.optimizer import ScheduledOptim
    pp, mc, tc, path = configs(levels)
    torch.manual_seed(0)
    model = fs2.FastSpeech2(pp, mc, path)
    mg.seeded(model)
    model.train()
    opt = ScheduledOptim(model, tc, mc, 0)
    Loss = loss_mod.FastSpeech2Loss(pp, mc)
    eLoss = loss_mod.SpeakerMetaEncLoss(pp, mc)
    batch = batch_for(B, Ts, levels)
    res = {"B": np.array(B), "Ts": np.array(Ts), "seed": np.array(SEED),
           "config": np.array("JVS-VCTK"), "pitch_level": np.array(levels[0]),
           "energy_level": np.array(levels[1]),
           "pos_enc_probe": model.encoder.position_enc.detach()[0, ::97, ::31].numpy()}
    for s in range(steps):
        output = model(*(batch[2:12]), accents=batch[13], speaker_meta=batch[12])
        losses = Loss(batch[:12], output[:-2])
        losses[0].backward()
        eloss = eLoss(output[-1], output[-2])
        (-eloss).backward()
        gn = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step_and_update_lr()
        opt.zero_grad()
        res[f"s{s}.losses"] = np.array([float(l) for l in losses])
        res[f"s{s}.eloss"] = np.array(float(eloss))
        res[f"s{s}.gnorm"] = np.array(float(gn))
        res[f"s{s}.lr"] = np.array(opt._optimizer.param_groups[0]["lr"])
        o, po = output[0].detach().double(), output[1].detach().double()
        res[f"s{s}.out_sum"] = np.array([o.sum(), o.abs().sum(), po.sum(), po.abs().sum()])
        res[f"s{s}.out_probe"] = output[1].detach()[:, ::37, ::7].numpy()
        preds = [output[i].detach().numpy() for i in (2, 3, 4)]
        res[f"s{s}.pred_probe"] = np.stack([p for p in preds if p.shape[1] == Ts])
        res[f"s{s}.frame_pred_probe"] = np.stack([p for p in preds if p.shape[1] != Ts])
        res[f"s{s}.mel_lens"] = output[9].numpy()
    res["final_probe"] = torch.cat([p.detach().reshape(-1)[:64] for p in model.parameters()
                                    if p.requires_grad]).numpy()
    np.savez_compressed(os.path.join(OUT, name), **res)
    print(name, res["s0.losses"], res["s2.losses"])


def g13(fs2, loss_mod, levels=("frame_level", "frame_level")):
    pp, mc, tc, path = configs(levels)
    torch.manual_seed(0)
    model = fs2.FastSpeech2(pp, mc, path)
    mg.seeded(model)
    ov = mg.infer_overrides()
    mg._apply(model, ov)
    model.eval()
    res = {"ov." + k: v for k, v in ov.items()}
    res.update(B=np.array(3), Ts=np.array(16), seed=np.array(SEED), p_control=np.array(1.3),
               d_control=np.array(1.2))

    def record(tag, out):
        for i, name in enumerate(("out", "post", "p", "e", "log_d", "d_r")):
            res[f"{tag}.{name}"] = out[i].detach().float().numpy()
        res[f"{tag}.mel_mask"] = out[7].numpy()
        res[f"{tag}.mel_lens"] = out[9].numpy()

    b = batch_for(3, 16, levels)
    with torch.no_grad():
        record("A", model(b[2], b[3], b[4], b[5], p_control=1.3, d_control=1.2, accents=b[13],
                          speaker_meta=b[12]))
        out = model(*(b[2:12]), accents=b[13], speaker_meta=b[12])
        record("B", out)
        losses = loss_mod.FastSpeech2Loss(pp, mc)(b[:12], out[:-2])
        res["B.losses"] = np.array([float(l) for l in losses])
    np.savez_compressed(os.path.join(OUT, "g13_frame_infer.npz"), **res)
    print("g13: mel lens A", res["A.mel_lens"], "B", res["B.mel_lens"], "losses", res["B.losses"])


def main():
    fs2, loss_mod, _, _ = mg.import_reference()
    mg.no_dropout()
    torch.set_num_threads(8)
    g12(fs2, loss_mod, ("frame_level", "frame_level"), "g12_frame_step_b3_t16.npz")
    g12(fs2, loss_mod, ("phoneme_level", "frame_level"), "g12_mixed_step_b3_t16.npz")
    g13(fs2, loss_mod)


if __name__ == "__main__":
    main()
