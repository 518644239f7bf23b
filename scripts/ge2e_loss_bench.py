"""fs2_ge2e_softmax and fs2_ge2e_contrast alone (the table of DESIGN.md section 7): loss only and
loss + gradients at N speakers x M = 10 utterances, D = 64; 100 calls between two events, 5
repeats, microseconds per call, sorted."""
import importlib, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K = importlib.import_module("mid-attribute-speaker-generation_amd.kernels")
dev = "cuda:0"
M, D, CALLS, REPS = 10, 64, 100, 5


def timeit(run):
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(CALLS):
            run()
        e.record()
        torch.cuda.synchronize()
        out.append(round(s.elapsed_time(e) / CALLS * 1e3, 2))
    return sorted(out)


w, b, g = (torch.tensor(v, device=dev) for v in (10.0, -5.0, 1.0))
for N in (4, 32, 64):  # 32 x 10 is the reference's training batch
    gen = torch.Generator().manual_seed(N)
    e = torch.randn(N, M, D, generator=gen) + 1.5 * torch.randn(N, 1, D, generator=gen)
    e = (e / e.norm(dim=2, keepdim=True)).to(dev)
    for name, fn in (("softmax", K.ge2e_softmax), ("contrast", K.ge2e_contrast)):
        print(f"{N} x {M} x {D} {name}: loss only {timeit(lambda: fn(e, w, b))} us, "
              f"loss + gradients {timeit(lambda: fn(e, w, b, g=g, grads=True))} us", flush=True)
