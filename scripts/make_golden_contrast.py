"""Captures the GE2E contrast-loss fixture from the *reference itself*: its ``utils.get_similarity``
+ ``get_contrast_loss`` under torch autograd in float64, at ``S = w sim + b`` with w = 10, b = -5
(speech_embedder_net.py:173-179), on the seeded inputs of ``tests/contrast_oracle.py``.  Run in the
build container (``python scripts/make_golden_contrast.py``); no test calls it and only data
leaves it.

  g18_contrast.npz
    shapes (4, 3), seeds (4)      the (N, M, D) cases and the seed of each
    c{k}.loss, c{k}.demb, c{k}.dw, c{k}.db   float64
"""
import os
import sys
from importlib import import_module

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import make_golden as mg  # noqa: E402
import contrast_oracle as co  # noqa: E402


def reference_contrast(utils, e, w=10.0, b=-5.0):
    """loss, demb, dw, db of the reference's own functions in float64."""
    et = torch.from_numpy(np.asarray(e, dtype=np.float64)).requires_grad_()
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    loss = utils.get_contrast_loss(wt * utils.get_similarity(et) + bt)
    loss.backward()
    return loss.item(), et.grad.numpy(), wt.grad.item(), bt.grad.item()


def main():
    sen = mg.import_discriminator()
    utils = import_module(sen.__package__ + ".utils")
    res = {"shapes": np.array(co.CPU_SHAPES), "seeds": np.array([co.SEEDS[s] for s in co.CPU_SHAPES])}
    for k, shape in enumerate(co.CPU_SHAPES):
        e = co.make_embeddings(*shape, co.SEEDS[shape])
        loss, demb, dw, db = reference_contrast(utils, e)
        res[f"c{k}.loss"], res[f"c{k}.demb"] = np.float64(loss), demb
        res[f"c{k}.dw"], res[f"c{k}.db"] = np.float64(dw), np.float64(db)
        print(shape, loss, dw, db)
    path = os.path.join(mg.OUT, "g18_contrast.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
