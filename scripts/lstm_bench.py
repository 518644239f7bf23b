"""One LSTM layer (N=192 sequences x 150 steps, H=256) forward / backward alone."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
from importlib import import_module
lib = import_module("mid-attribute-speaker-generation_amd._lib").lib
dev = "cuda:0"
N, T, H, D = 192, 150, 256, 256
x = torch.randn(N * T, D, device=dev)
w_ih = torch.randn(4 * H, D, device=dev) * 0.05
w_hh = torch.randn(4 * H, H, device=dev) * 0.05
bias = torch.randn(4 * H, device=dev) * 0.05
w_hh_t = w_hh.t().contiguous()
w_ih_t = w_ih.t().contiguous()
gx = torch.empty(N * T, 4 * H, device=dev)
h = torch.empty(N * T, H, device=dev)
c = torch.empty(N * T, H, device=dev)
act = torch.empty(N * T, 4 * H, device=dev)
dh = torch.randn(N * T, H, device=dev) * 0.01
dg = torch.empty(N * T, 4 * H, device=dev)
dc = torch.empty(2 * N * H, device=dev)
dx = torch.empty(N * T, D, device=dev)
P = lambda t: t.data_ptr()


def fwd():
    lib.fs2_lstm_layer_fwd(P(x), N, T, D, H, P(w_ih), P(bias), P(w_hh), P(gx), P(h), P(c), P(act), K.stream())


def bwd():
    lib.fs2_lstm_layer_bwd(P(dh), N, T, D, H, P(w_ih_t), P(w_hh_t), P(act), P(c), P(dg), P(dc), P(dx), K.stream())


def timeit(run, n=5):
    run()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


def wgrad_leg(n_seq, steps, L=3, c_in=80, n=10):
    """--wgrad: the GE2E stack (80 -> 256 x 3) forward, backward and weight gradients alone at
    n_seq x steps rows; FLOPs of the weight gradient = 2 rows 4H (c_in_l + H) summed over l."""
    rows = n_seq * steps
    xs = torch.randn(rows, c_in, device=dev)
    wi0 = torch.randn(4 * H, c_in, device=dev) * 0.05
    wiu = torch.randn(L - 1, 4 * H, H, device=dev) * 0.05
    wh = torch.randn(L, 4 * H, H, device=dev) * 0.05
    b = torch.randn(L, 4 * H, device=dev) * 0.05
    wi0_t, wiu_t, wh_t = wi0.t().contiguous(), wiu.transpose(1, 2).contiguous(), wh.transpose(1, 2).contiguous()
    g = torch.empty(rows, 4 * H, device=dev)
    hs, cs = torch.empty(L, rows, H, device=dev), torch.empty(L, rows, H, device=dev)
    a, dgs = torch.empty(L, rows, 4 * H, device=dev), torch.empty(L, rows, 4 * H, device=dev)
    dcs, dxs = torch.empty(L * 2 * n_seq * H, device=dev), torch.empty(rows, c_in, device=dev)
    dhs = torch.randn(rows, H, device=dev) * 0.01
    outs = [torch.empty(4 * H, c_in, device=dev), torch.empty(L - 1, 4 * H, H, device=dev),
            torch.empty(L, 4 * H, H, device=dev), torch.empty(L, 4 * H, device=dev)]
    nb = lib.fs2_lstm_stack_wgrad_ws_bytes(n_seq, steps, c_in, H, L)
    ws = torch.empty(nb // 4, device=dev)
    f = lambda: lib.fs2_lstm_stack_fwd(P(xs), n_seq, steps, c_in, H, L, P(wi0), P(wiu), P(wh), P(b),
                                       P(g), P(hs), P(cs), P(a), K.stream())
    bw = lambda: lib.fs2_lstm_stack_bwd(P(dhs), n_seq, steps, c_in, H, L, P(wi0_t), P(wiu_t),
                                        P(wh_t), P(a), P(cs), P(dgs), P(dcs), P(dxs), K.stream())
    wg = lambda: lib.fs2_lstm_stack_wgrad(P(xs), P(hs), P(dgs), n_seq, steps, c_in, H, L,
                                          *[P(t) for t in outs], 0, P(ws), nb, K.stream())
    tf, tb, tw = timeit(f, n), timeit(bw, n), timeit(wg, n)
    flop = 2.0 * rows * 4 * H * ((c_in + H) + (L - 1) * 2 * H)
    print(f"stack {n_seq} x {steps}: fwd {tf:.3f} ms, bwd {tb:.3f} ms, wgrad {tw:.3f} ms "
          f"({flop / 1e9:.1f} GF, {flop / tw / 1e9:.1f} TF/s, "
          f"{100 * flop / tw / 1e9 / 155:.1f}% of the 155 TF f32-MFMA peak; "
          f"workspace {nb / 2 ** 20:.1f} MiB)", flush=True)


if "--wgrad" in sys.argv:
    wgrad_leg(320, 150)  # N M = 32 x 10, the reference's training batch
    wgrad_leg(192, 150)
    sys.exit(0)

if os.environ.get("LSTM_PROBE"):  # PMC probe: only the stacked kernels, a few launches
    L = 3
    w_ih_up = torch.randn(L - 1, 4 * H, H, device=dev) * 0.05
    w_hh3 = torch.randn(L, 4 * H, H, device=dev) * 0.05
    bias3 = torch.randn(L, 4 * H, device=dev) * 0.05
    w_ih_up_t, w_hh3_t = w_ih_up.transpose(1, 2).contiguous(), w_hh3.transpose(1, 2).contiguous()
    h3, c3 = torch.empty(L, N * T, H, device=dev), torch.empty(L, N * T, H, device=dev)
    act3, dg3 = torch.empty(L, N * T, 4 * H, device=dev), torch.empty(L, N * T, 4 * H, device=dev)
    dc3 = torch.empty(L * 2 * N * H, device=dev)
    lib.fs2_lstm_stack_fwd(P(x), N, T, D, H, L, P(w_ih), P(w_ih_up), P(w_hh3), P(bias3), P(gx),
                           P(h3), P(c3), P(act3), K.stream())
    lib.fs2_lstm_stack_bwd(P(dh), N, T, D, H, L, P(w_ih_t), P(w_ih_up_t), P(w_hh3_t), P(act3),
                           P(c3), P(dg3), P(dc3), P(dx), K.stream())
    torch.cuda.synchronize()
    sys.exit(0)

# reference: torch LSTM cell recurrence (fp32) on the same weights, for a correctness check
fwd()
torch.cuda.synchronize()
lstm = torch.nn.LSTM(D, H, batch_first=True).to(dev)
with torch.no_grad():
    lstm.weight_ih_l0.copy_(w_ih); lstm.weight_hh_l0.copy_(w_hh)
    lstm.bias_ih_l0.copy_(bias); lstm.bias_hh_l0.zero_()
xr = x.view(N, T, D).clone().requires_grad_(True)
ref, _ = lstm(xr)
print("fwd max abs err vs torch", (h.view(N, T, H) - ref.detach()).abs().max().item(), flush=True)
ref.backward(dh.view(N, T, H))
bwd()
torch.cuda.synchronize()
print("bwd dx max abs err vs torch", (dx.view(N, T, D) - xr.grad).abs().max().item(),
      "ref max", xr.grad.abs().max().item(), flush=True)
print(f"layer fwd {timeit(fwd):.3f} ms, bwd {timeit(bwd):.3f} ms", flush=True)


# the 3-layer stack: per-layer path vs the wavefront entry points
L = 3
w_ih_up = torch.randn(L - 1, 4 * H, H, device=dev) * 0.05
w_hh3 = torch.randn(L, 4 * H, H, device=dev) * 0.05
bias3 = torch.randn(L, 4 * H, device=dev) * 0.05
w_ih_up_t, w_hh3_t = w_ih_up.transpose(1, 2).contiguous(), w_hh3.transpose(1, 2).contiguous()
h3, c3 = torch.empty(L, N * T, H, device=dev), torch.empty(L, N * T, H, device=dev)
act3, dg3 = torch.empty(L, N * T, 4 * H, device=dev), torch.empty(L, N * T, 4 * H, device=dev)
dc3 = torch.empty(L * 2 * N * H, device=dev)
dh3 = torch.randn(N * T, H, device=dev) * 0.01


def sfwd():
    lib.fs2_lstm_stack_fwd(P(x), N, T, D, H, L, P(w_ih), P(w_ih_up), P(w_hh3), P(bias3), P(gx),
                           P(h3), P(c3), P(act3), K.stream())


def sbwd():
    lib.fs2_lstm_stack_bwd(P(dh3), N, T, D, H, L, P(w_ih_t), P(w_ih_up_t), P(w_hh3_t), P(act3),
                           P(c3), P(dg3), P(dc3), P(dx), K.stream())


print(f"3-layer stack (wavefront): fwd {timeit(sfwd):.3f} ms, bwd {timeit(sbwd):.3f} ms "
      f"(per-layer path: about 3x the layer times above plus 4 GEMMs)", flush=True)
