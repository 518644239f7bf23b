"""Captures the speaker-encoder training fixture from the *reference itself* (CPU, fp32, dropout
off, name-seeded weights), the way ``scripts/make_golden_frame_level.py`` captures g12 / g13.
Run in the build container (``python scripts/make_golden_embedder_train.py``); no test calls it
and only data leaves it.

  g14_embedder_train.npz
    x (9, 20, 80), langs (9)     N = 3 speakers x M = 3 utterances, T = 20 frames
    progress, threshold          train progress (> da_startpoint, so the da_loss < threshold
                                 test decides) and compute_da_threshold at N x M = 9
    {shipped,ge2e,da_only}.scalars  (steps, 5): loss, da_loss, norm_main, norm_ge2e, norm_da per
                                 step of the reference's loop body (train_speech_embedder.py:
                                 167-191 with the batch shuffle left out; ``ge2e`` is the same
                                 with line 181's ``loss.backward`` live; ``da_only`` is
                                 da_classifier_subroutine's body, 249-277, with 0 where that
                                 loop has no such scalar).  A norm whose clip the reference
                                 skips is 0.
    {shipped,ge2e}.gate          (steps): 1 where da_loss.backward() ran
    emb, logits                  step-0 forward
    {shipped,ge2e}.grad.<name>   step-0 gradient before clipping: in full for tensors of at most
                                 16,384 elements, else 4,096 entries at ``idx.<name>``;
                                 ``.gmax`` / ``.gl2``: its max-abs and L2 norm
    sd.keys, sd.shapes, ge2e.keys  the checkpoint's {'embedder_net', 'ge2e'} layout
    loss{k}.{emb,loss,demb,dw,db}  GE2ELoss on random unit embeddings at (N, M) = (3,3), (4,2),
                                 (2,5), D = 64
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import make_golden as mg  # noqa: E402

N, M, T, STEPS, DA_STEPS = 3, 3, 20, 3, 2
PROGRESS = 0.5
FULL, SAMPLES = 16384, 4096
LOSS_CASES = ((3, 3), (4, 2), (2, 5))


def fresh(sen):
    torch.manual_seed(0)
    net = sen.SpeechEmbedder()
    mg.seeded(net)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    net.train()
    crit = sen.GE2ELoss("cpu")
    opt = torch.optim.Adam
    optimizers = {"main": opt(net.main_parameters(), lr=1e-3, weight_decay=1e-6),
                  "ge2e": opt(crit.parameters(), lr=1e-3),
                  "da": opt(net.da_parameters(), 1e-3, weight_decay=1e-6)}
    return net, crit, optimizers


def record_grads(res, tag, net, crit):
    named = list(net.named_parameters()) + [("ge2e." + k, p) for k, p in crit.named_parameters()]
    for name, p in named:
        g = torch.zeros_like(p) if p.grad is None else p.grad.detach()
        g = g.reshape(-1).numpy()
        res[f"{tag}.grad.{name}.gmax"] = np.float64(np.abs(g).max())
        res[f"{tag}.grad.{name}.gl2"] = np.float64(np.sqrt((g.astype(np.float64) ** 2).sum()))
        if g.size <= FULL:
            res[f"{tag}.grad.{name}"] = g.reshape(p.shape).copy()
        else:
            idx = np.sort(np.random.default_rng(g.size + len(name)).integers(0, g.size,
                                                                             size=SAMPLES))
            res[f"idx.{name}"] = idx.astype(np.int32)  # sorted: they deflate well
            res[f"{tag}.grad.{name}"] = g[idx].copy()


def trajectory(sen, x, langs, threshold, ge2e_backward, res, tag):
    clip = torch.nn.utils.clip_grad_norm_
    net, crit, opts = fresh(sen)
    scal, gates = [], []
    for s in range(STEPS):
        for o in opts.values():
            o.zero_grad()
        out = net(x)
        emb, logits = out["embeddings"], out["da_lang_logits"]
        if s == 0:
            res["emb"], res["logits"] = emb.detach().numpy(), logits.detach().numpy()
        _, loss, da_loss = crit(emb.reshape(N, M, -1), logits, langs)
        da_on = bool(da_loss < threshold) or PROGRESS <= sen.hp.model.da_startpoint
        if ge2e_backward:
            loss.backward(retain_graph=da_on)
        if da_on:
            da_loss.backward()
        if s == 0:
            record_grads(res, tag, net, crit)
        n_main = clip(net.main_parameters(), 3.0)
        n_ge2e = clip(crit.parameters(), 1.0)
        opts["main"].step()
        opts["ge2e"].step()
        n_da = 0.0
        if da_on:
            n_da = clip(net.da_parameters(), 3.0)
            opts["da"].step()
        scal.append([float(loss), float(da_loss), float(n_main), float(n_ge2e), float(n_da)])
        gates.append(float(da_on))
    res[f"{tag}.scalars"], res[f"{tag}.gate"] = np.array(scal), np.array(gates)
    print(tag, np.array(scal), gates)


def da_only(sen, x, langs, res):
    import torch.nn.functional as F
    net, crit, opts = fresh(sen)
    before = [p.detach().clone() for p in net.main_parameters()]
    scal = []
    for s in range(DA_STEPS):
        opts["da"].zero_grad()
        out = net(x, detach=True)
        da_loss = F.binary_cross_entropy_with_logits(out["da_lang_logits"], langs, reduction="sum")
        da_loss.backward()
        n_da = torch.nn.utils.clip_grad_norm_(net.da_classifier.parameters(), 3.0)
        opts["da"].step()
        scal.append([0.0, float(da_loss), 0.0, 0.0, float(n_da)])
    assert all(torch.equal(a, b) for a, b in zip(before, net.main_parameters()))
    res["da_only.scalars"] = np.array(scal)
    print("da_only", np.array(scal))


def loss_cases(sen, res):
    for k, (n, m) in enumerate(LOSS_CASES):
        rng = np.random.default_rng(140 + k)
        e = rng.standard_normal((n, m, 64))
        e = (e / np.linalg.norm(e, axis=2, keepdims=True)).astype(np.float32)
        crit = sen.GE2ELoss("cpu")
        et = torch.from_numpy(e).requires_grad_()
        _, loss, _ = crit(et, None, None)
        loss.backward()
        res[f"loss{k}.emb"], res[f"loss{k}.loss"] = e, np.float64(loss.item())
        res[f"loss{k}.demb"] = et.grad.numpy()
        res[f"loss{k}.dw"], res[f"loss{k}.db"] = (np.float64(crit.w.grad.item()),
                                                  np.float64(crit.b.grad.item()))
        print(f"loss{k}", (n, m), loss.item(), crit.w.grad.item(), crit.b.grad.item())


def main():
    sen = mg.import_discriminator()
    torch.set_num_threads(8)
    sen.hp.train.N, sen.hp.train.M = N, M
    from importlib import import_module
    utils = import_module(sen.__package__ + ".utils")
    threshold = utils.compute_da_threshold(sen.hp)
    rng = np.random.default_rng(12)
    x = torch.from_numpy((rng.standard_normal((N * M, T, 80)) * 2 - 3).astype(np.float32))
    langs = torch.tensor([1., 1., 1., 0., 0., 0., 1., 1., 1.])
    net, crit, _ = fresh(sen)
    sd = net.state_dict()
    res = {"x": x.numpy(), "langs": langs.numpy(), "progress": np.float64(PROGRESS),
           "threshold": np.float64(threshold), "N": np.array(N), "M": np.array(M),
           "sd.keys": np.array(list(sd.keys())),
           "sd.shapes": np.array([",".join(map(str, v.shape)) for v in sd.values()]),
           "ge2e.keys": np.array(list(crit.state_dict().keys()))}
    trajectory(sen, x, langs, threshold, False, res, "shipped")
    trajectory(sen, x, langs, threshold, True, res, "ge2e")
    da_only(sen, x, langs, res)
    loss_cases(sen, res)
    path = os.path.join(mg.OUT, "g14_embedder_train.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
