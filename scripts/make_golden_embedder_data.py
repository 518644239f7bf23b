"""Captures the speaker-encoder data-path fixture from the *reference itself*: its own
``SpeakerDataset`` / ``Collate`` (data_load.py) over a synthetic corpus, and its own
``get_centroids`` / ``get_cossim`` (utils.py), the way ``make_golden_embedder_train.py`` captures
g14.  Run in the build container (``python scripts/make_golden_embedder_data.py``); no test
calls it and only data leaves it.

  g15_embedder_data.npz
    seed, files                  the ``random.seed`` and the file order the reference's glob saw
                                 (the corpus is ``tests/embedder_data_oracle.write_corpus``:
                                 every element encodes its file, utterance, channel and frame)
    batch{0,1}.{L,langs,first,last,next}
                                 two consecutive batches of DataLoader(batch_size=4,
                                 shuffle=False, drop_last=True, collate_fn=Collate(True)) at
                                 M = 3, each followed by the training loop's
                                 ``random.shuffle`` of 12 indices (train_speech_embedder.py:
                                 160-161): the crop length, the collated langs, each row's
                                 element [0, 0] and [L - 1, 79], and the ``random.random()``
                                 the generator would give next
    spk.{seed,index,L,langs,first,last,next}
                                 get_spkr2embedding's batch (289-295) of file ``index``:
                                 shuffle=False, utter_num=400, Collate()
    eer{0,1,2,3}.{enroll,verify,sim,result}
                                 unit embeddings, D = 64, (N, m_enr, m_ver) = (5, 2, 4),
                                 (4, 3, 3), (2, 1, 2) drawn as normalize(base + 0.5 own_spk +
                                 0.5 noise), and a degenerate (3, 2, 2) of unrelated vectors
                                 whose sims are all below 0.5; ``sim`` is the reference's
                                 get_cossim(verify, get_centroids(enroll)); ``result`` = EER,
                                 threshold, FAR, FRR of the sweep over it (float32).  Seeds are
                                 drawn until every sim is >= 1e-4 from every threshold and at
                                 least two cases have an interior threshold with EER > 0.
"""
import os
import random
import sys
import tempfile
from importlib import import_module

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from oracle import make_golden as mg  # noqa: E402
import embedder_data_oracle as O  # noqa: E402

SEED, N, M = 15, 4, 3
SPK_INDEX, UTTER_NUM = 2, 400
EER_CASES = ((5, 2, 4), (4, 3, 3), (2, 1, 2))
GAP = 1e-4


def rows_first_last(mels):
    """mels (rows, L, 80) -> each row's first and last element."""
    m = mels.reshape(-1, mels.shape[-2], mels.shape[-1]).numpy()
    return m[:, 0, 0].copy(), m[:, -1, -1].copy()


def peek():
    state = random.getstate()
    nxt = random.random()
    random.setstate(state)
    return np.float64(nxt)


def batches(sen, res):
    pkg = sen.__package__
    # data_load.py imports its siblings by their top-level names
    sys.modules["hparam"] = sys.modules[pkg + ".hparam"]
    sys.modules["utils"] = import_module(pkg + ".utils")
    dl = import_module(pkg + ".data_load")
    hp = sen.hp
    from torch.utils.data import DataLoader
    with tempfile.TemporaryDirectory() as tmp:
        O.write_corpus(tmp)
        hp.training = True
        hp.data.train_path = tmp
        hp.train.N, hp.train.M = N, M
        ds = dl.SpeakerDataset()
        res["seed"] = np.array(SEED)
        res["files"] = np.array(ds.file_list)
        assert sorted(ds.file_list) == list(O.NAMES)
        random.seed(SEED)
        loader = DataLoader(ds, batch_size=N, shuffle=False, num_workers=0, drop_last=True,
                            collate_fn=dl.Collate(True))
        it = iter(loader)
        for b in range(2):
            try:
                batch = next(it)
            except StopIteration:  # one batch per epoch of 6 files: the next epoch's loader
                it = iter(loader)
                batch = next(it)
            mels = batch["mels"]
            assert mels.shape[:2] == (N, M) and mels.shape[3] == O.NMELS
            perm = list(range(N * M))
            random.shuffle(perm)
            first, last = rows_first_last(mels)
            res[f"batch{b}.L"] = np.array(mels.shape[2])
            res[f"batch{b}.langs"] = batch["langs"].numpy()
            res[f"batch{b}.first"], res[f"batch{b}.last"] = first, last
            res[f"batch{b}.next"] = peek()
            print("batch", b, "L", mels.shape[2], O.decode(first)[:2], batch["langs"])
        # get_spkr2embedding
        ds.shuffle = False
        ds.utter_num = UTTER_NUM
        random.seed(SEED + 1)
        ds_item = dl.Collate()([ds[SPK_INDEX]])  # the loader's batch_size=1 batch of that index
        mels = ds_item["mels"].squeeze(0)
        first, last = rows_first_last(mels)
        res["spk.seed"], res["spk.index"] = np.array(SEED + 1), np.array(SPK_INDEX)
        res["spk.L"] = np.array(mels.shape[1])
        res["spk.langs"] = ds_item["langs"].numpy()
        res["spk.first"], res["spk.last"], res["spk.next"] = first, last, peek()
        print("spk", mels.shape, ds_item["langs"][:3])


def draw(rng, n, me, mv, related):
    """(enroll (n, me, 64), verify (n, mv, 64)) unit vectors: normalize(base + 0.5 own_spk +
    0.5 noise), or unrelated noise alone."""
    d = 64
    e = rng.standard_normal((n, me + mv, d))
    if related:
        e = rng.standard_normal(d) + 0.5 * rng.standard_normal((n, 1, d)) + 0.5 * e
    e = (e / np.linalg.norm(e, axis=2, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(e[:, :me]), np.ascontiguousarray(e[:, me:])


def eer_cases(utils, res):
    def ref_sim(enroll, verify):
        return utils.get_cossim(torch.from_numpy(verify),
                                utils.get_centroids(torch.from_numpy(enroll))).numpy()

    seed = 150
    while True:
        rng = np.random.default_rng(seed)
        got = []
        for n, me, mv in EER_CASES:
            enroll, verify = draw(rng, n, me, mv, True)
            sim = ref_sim(enroll, verify)
            got.append((enroll, verify, sim, O.eer_sweep(sim)[1]))
        ok = all(O.threshold_gap(g[2]) >= GAP for g in got)
        interior = sum(0.5 < float(g[3][1]) < 0.99 and float(g[3][0]) > 0 for g in got)
        if ok and interior >= 2:
            break
        seed += 1
        assert seed < 2150, "no seed found"
    print("eer seed", seed)
    seed_d = 0
    while True:
        rng = np.random.default_rng(1500 + seed_d)
        enroll, verify = draw(rng, 3, 2, 2, False)
        sim = ref_sim(enroll, verify)
        if sim.max() < 0.5 - GAP:
            break
        seed_d += 1
        assert seed_d < 2000, "no seed found"
    got.append((enroll, verify, sim, O.eer_sweep(sim)[1]))
    assert not got[-1][3].any()
    for k, (enroll, verify, sim, result) in enumerate(got):
        # the sweep once more with torch's fp32 tensor arithmetic (counts, then divisions)
        s = torch.from_numpy(sim)
        n, mv, _ = sim.shape
        own = torch.eye(n, dtype=torch.bool)[:, None, :]
        best = None
        for thr in O.thresholds():
            on = s > float(thr)
            accepted, same = on.sum().float(), (on & own).sum().float()
            far = (accepted - same) / (n - 1.0) / float(mv) / n
            frr = (n * mv - same) / float(mv) / n
            if (best[0] if best else 1) > abs(far - frr):
                best = (abs(far - frr), (far + frr) / 2, thr, far, frr)
        want = np.array([float(x) for x in best[1:]], np.float32) if best else np.zeros(4, np.float32)
        assert np.array_equal(want, result), (want, result)
        res[f"eer{k}.enroll"], res[f"eer{k}.verify"] = enroll, verify
        res[f"eer{k}.sim"], res[f"eer{k}.result"] = sim, result
        print(f"eer{k}", sim.shape, result, "gap", O.threshold_gap(sim))


def main():
    sen = mg.import_discriminator()
    torch.set_num_threads(4)
    res = {}
    batches(sen, res)
    eer_cases(sys.modules["utils"], res)
    path = os.path.join(mg.OUT, "g15_embedder_data.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
