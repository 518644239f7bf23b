"""The ``rescnn`` speaker encoder, the parts that need no GPU: the test oracle against an
independent composition of ``torch.nn`` modules, the module's state-dict layout (the
reference's keys, aliases included), and the new entry points' argument checks."""
import importlib

import pytest
import torch
import torch.nn as nn

import rescnn_oracle as O

G = importlib.import_module("mid-attribute-speaker-generation_amd.ge2e")
L = importlib.import_module("mid-attribute-speaker-generation_amd._lib")

LSTM_KEYS = [f"LSTM_stack.{n}_l{l}" for l in range(3)
             for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
HEAD_KEYS = [f"{p}.{k}" for p in ["projection.linear_layer"] + [
    f"da_classifier.classifier.layer.linear_{i}.linear_layer" for i in range(3)]
    for k in ("weight", "bias")]
CN = ("conv.weight", "conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var",
      "bn.num_batches_tracked")


def expected_rescnn_keys():
    own, seq = [], []
    for i in range(1, 5):
        own += [f"conv{i}.{k}" for k in CN]
        own += [f"res{i}.{c}.{k}" for c in ("conv1", "conv2") for k in CN]
        seq += [f"conv_layer.{3 * (i - 1)}.{k}" for k in CN]
        seq += [f"conv_layer.{3 * (i - 1) + 2}.{c}.{k}" for c in ("conv1", "conv2") for k in CN]
    return ["_feat_extractor." + k for k in own + seq] + HEAD_KEYS


def randomised(seed=0):
    """A CPU module whose BatchNorm parameters and buffers are not at their initial values."""
    torch.manual_seed(seed)
    m = G.SpeechEmbedder("cpu", architecture="rescnn")
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("bn.weight"):
                v.uniform_(0.5, 1.5)
            elif k.endswith(("bn.bias", "running_mean", "conv.bias")):
                v.uniform_(-0.3, 0.3)
            elif k.endswith("running_var"):
                v.uniform_(0.5, 2.0)
    return m


class TorchNet(nn.Module):
    """The same network from ``nn.Conv2d`` / ``nn.BatchNorm2d`` (float64)."""

    def __init__(self, sd):
        super().__init__()
        self.cn = nn.ModuleList()
        for pre, k, stride, _ in O.layer_names():
            w = sd[pre + "conv.weight"]
            conv = nn.Conv2d(w.shape[1], w.shape[0], k, stride, k // 2)
            bn = nn.BatchNorm2d(w.shape[0])
            conv.load_state_dict({"weight": w, "bias": sd[pre + "conv.bias"]})
            bn.load_state_dict({n: sd[pre + "bn." + n] for n in
                                ("weight", "bias", "running_mean", "running_var",
                                 "num_batches_tracked")})
            self.cn.append(nn.Sequential(conv, bn))
        self.double()

    def forward(self, x):
        a = x.double().transpose(1, 2).unsqueeze(1)
        for i in range(0, 12, 3):
            a = torch.relu(self.cn[i](a))
            a = torch.relu(self.cn[i + 2](torch.relu(self.cn[i + 1](a))) + a)
        return nn.functional.adaptive_avg_pool2d(a, (None, 1)).view(a.shape[0], -1)


@pytest.mark.parametrize("training", (True, False))
def test_oracle_matches_torch_modules(training):
    m = randomised()
    sd = m.state_dict()
    x = torch.randn(3, 19, 80)
    orc, net = O.Oracle(sd), TorchNet(sd)
    net.train(training)
    feat = O.pool_flatten(orc.features(x, training))
    want = net(x)
    assert feat.shape == want.shape == (3, 640)
    assert (feat - want).abs().max() <= 1e-12 * want.abs().max()
    g = torch.randn(3, 640, dtype=torch.float64)
    (feat * g).sum().backward()
    (want * g).sum().backward()
    for i, (pre, _, _, _) in enumerate(O.layer_names()):
        conv, bn = net.cn[i]
        for name, p in (("conv.weight", conv.weight), ("conv.bias", conv.bias),
                        ("bn.weight", bn.weight), ("bn.bias", bn.bias)):
            got = orc.par[pre + name].grad
            if training and name == "conv.bias":  # zero in exact arithmetic (BN removes the mean)
                bound = 1e-9
            else:
                bound = 1e-10 * max(p.grad.abs().max().item(), 1e-3)
            assert (got - p.grad).abs().max() <= bound, (pre, name)
        for name in ("running_mean", "running_var"):
            assert torch.allclose(orc.buf[pre + "bn." + name], getattr(bn, name), rtol=1e-12,
                                  atol=1e-14)
        assert orc.buf[pre + "bn.num_batches_tracked"] == bn.num_batches_tracked == int(training)


def test_oracle_float32_switch_and_head():
    m = randomised(1)
    x = torch.randn(2, 19, 80)
    o64, o32 = O.Oracle(m.state_dict()), O.Oracle(m.state_dict(), torch.float32)
    a, b = o64.forward(x), o32.forward(x)
    assert b["embeddings"].dtype == torch.float32 and a["embeddings"].dtype == torch.float64
    assert torch.allclose(a["embeddings"].norm(dim=1), torch.ones(2, dtype=torch.float64))
    assert (a["embeddings"] - b["embeddings"]).abs().max() < 1e-4
    assert a["da_lang_logits"].shape == (2,)
    # the channel-major flatten: feature c * 5 + h
    fm = torch.arange(2 * 128 * 5 * 3, dtype=torch.float64).view(2, 128, 5, 3)
    assert O.pool_flatten(fm)[1, 7 * 5 + 2] == fm[1, 7, 2].mean()


def test_state_dict_is_the_reference_layout():
    m = G.SpeechEmbedder("meta", architecture="rescnn")
    sd = m.state_dict()
    assert list(sd) == expected_rescnn_keys() and len(sd) == 176
    assert not any(k.startswith("LSTM_stack") for k in sd)
    fe = "_feat_extractor."
    widths, c_in = (16, 32, 64, 128), 1
    for i, c in enumerate(widths, 1):
        assert sd[f"{fe}conv{i}.conv.weight"].shape == (c, c_in, 5, 5)
        for blk in ("conv1", "conv2"):
            assert sd[f"{fe}res{i}.{blk}.conv.weight"].shape == (c, c, 3, 3)
        for pre in (f"conv{i}", f"res{i}.conv1", f"res{i}.conv2"):
            for k in CN[1:6]:
                assert sd[f"{fe}{pre}.{k}"].shape == (c,)
            nbt = sd[f"{fe}{pre}.bn.num_batches_tracked"]
            assert nbt.shape == () and nbt.dtype == torch.int64
        c_in = c
    assert sd["projection.linear_layer.weight"].shape == (64, 640)
    # the Sequential's entries are the same tensors
    real = G.SpeechEmbedder("cpu", architecture="rescnn").state_dict()
    for i in range(1, 5):
        for k in CN:
            assert real[f"{fe}conv_layer.{3 * (i - 1)}.{k}"].data_ptr() == \
                real[f"{fe}conv{i}.{k}"].data_ptr()
            for blk in ("conv1", "conv2"):
                assert real[f"{fe}conv_layer.{3 * (i - 1) + 2}.{blk}.{k}"].data_ptr() == \
                    real[f"{fe}res{i}.{blk}.{k}"].data_ptr()
    named = list(m.named_parameters())
    assert len(named) == 56 and len({id(p) for _, p in named}) == 56
    assert len(m.main_parameters()) == 50 and len(m.da_parameters()) == 6
    ids = {id(p) for p in m.main_parameters()} | {id(p) for p in m.da_parameters()}
    assert ids == {id(p) for p in m.parameters()}
    assert m.feat_dropout == 0.5 and m.da_dropout == 0.2


def test_state_dict_loads_into_reference_keys_roundtrip():
    a, b = randomised(2), G.SpeechEmbedder("cpu", architecture="rescnn")
    b.load_state_dict(a.state_dict())
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_lstm_architecture_is_unchanged_and_others_raise():
    for m in (G.SpeechEmbedder("meta"), G.SpeechEmbedder("meta", False, "LSTM")):
        sd = m.state_dict()
        assert list(sd) == LSTM_KEYS + HEAD_KEYS
        assert sd["projection.linear_layer.weight"].shape == (64, 256)
        assert len(m.main_parameters()) == 14
        assert not hasattr(m, "_feat_extractor")
    with pytest.raises(ValueError):
        G.SpeechEmbedder("meta", architecture="resnet")


def test_trainer_arenas_take_a_rescnn_embedder():
    T = importlib.import_module("mid-attribute-speaker-generation_amd.embedder_train")
    e = G.SpeechEmbedder("meta", True, "rescnn")
    tr = T.EmbedderTrainer(embedder=e, device="meta", n_utt=3)
    assert tr.optimizers["main"].arena.numel == sum(p.numel() for p in e.main_parameters())
    assert list(tr.state_dict()["embedder_net"]) == expected_rescnn_keys()


def test_new_entries_validate_arguments_before_any_launch():
    """FS2_ERR_ARG paths return before a stream is touched, so they run without a GPU."""
    lib, p, big = L.lib, 16, 1 << 30  # p: a non-null, aligned placeholder, never dereferenced
    bad = L.KernelError

    def conv(n=3, w=13, h=10, ci=16, co=32, k=5, s=2, pad=2):
        return lib.fs2_conv2d_fwd(p, n, w, h, ci, p, p, co, k, s, pad, None, None, None, 0, p, 0)

    for kw in (dict(ci=8), dict(ci=24), dict(co=24), dict(n=0), dict(w=0), dict(k=4), dict(s=3),
               dict(k=9), dict(w=1, h=1, k=5, pad=1)):
        with pytest.raises(bad):
            conv(**kw)
    with pytest.raises(bad):  # scale without shift
        lib.fs2_conv2d_fwd(p, 3, 13, 10, 16, p, p, 32, 5, 2, 2, p, None, None, 0, p, 0)
    with pytest.raises(bad):
        lib.fs2_conv2d_dgrad(p, 3, 13, 10, 12, p, 32, 5, 2, 2, None, p, 0)
    with pytest.raises(bad):
        lib.fs2_conv2d_dgrad(p, 0, 13, 10, 16, p, 32, 5, 2, 2, None, p, 0)
    with pytest.raises(bad):
        lib.fs2_conv2d_weight_prep(p, 20, 16, 3, p, p, 0)
    need = lib.fs2_conv2d_wgrad_ws_bytes(3, 13, 10, 16, 32, 5, 2, 2)
    assert need >= 25 * 16 * 32 * 4 and lib.fs2_conv2d_wgrad_ws_bytes(0, 13, 10, 16, 32, 5, 2, 2) == 0
    for kw in (dict(ws=need - 4), dict(n=0), dict(co=40), dict(beta=2)):
        a = dict(n=3, co=32, beta=0, ws=big)
        a.update(kw)
        with pytest.raises(bad):
            lib.fs2_conv2d_wgrad(p, p, a["n"], 13, 10, 16, a["co"], 5, 2, 2, p, p, a["beta"], p,
                                 a["ws"], 0)
    need = lib.fs2_bn2d_ws_bytes(105, 16)
    assert need == (2 * 1 * 16 + 2 * 16) * 4 and lib.fs2_bn2d_ws_bytes(257, 16) > need
    for rows, c, ws in ((105, 12, big), (105, 20, big), (0, 16, big), (105, 16, need - 4)):
        with pytest.raises(bad):
            lib.fs2_bn2d_fwd(p, rows, c, p, p, 1e-5, 0.1, p, p, p, p, p, None, 1, p, p, ws, 0)
        with pytest.raises(bad):
            lib.fs2_bn2d_bwd(p, p, p, p, p, p, rows, c, 1, p, p, p, p, p, ws, 0)
    with pytest.raises(bad):
        lib.fs2_pool_drop_fwd(p, 0, 2, 5, 128, 0.0, None, 1, p, 0)
    with pytest.raises(bad):  # dropout without a seed
        lib.fs2_pool_drop_fwd(p, 4, 2, 5, 128, 0.5, None, 1, p, 0)
    with pytest.raises(bad):
        lib.fs2_pool_drop_bwd(p, 4, 0, 5, 128, 0.0, None, 1, p, 0)
    head = (p,) * 11
    with pytest.raises(bad):  # width not a multiple of 64
        lib.fs2_clf_head_w(p, 600, 4, 600, *head, 0.0, None, 1, p, p, None, None, None, 0, 0)
    with pytest.raises(bad):  # dropout without a seed
        lib.fs2_clf_head_w(p, 640, 4, 640, *head, 0.2, None, 1, p, p, None, None, None, 0, 0)
    need = lib.fs2_clf_head_w_wgrad_ws_bytes(9)
    assert need > 0
    outs = (p,) * 8
    with pytest.raises(bad):
        lib.fs2_clf_head_w_wgrad(p, 640, 9, 640, *head, 0.0, None, 1, p, p, *outs, 0, p, need - 4, 0)
    with pytest.raises(bad):
        lib.fs2_clf_head_w_wgrad(p, 640, 9, 2048, *head, 0.0, None, 1, p, p, *outs, 0, p, big, 0)
