"""rth_fc_bwd beside another stream's launches (r07; the pattern of test_concurrency_gpu.py).  In
the Ape-X loop the learner's FC1 backward shares the CUs with the actor block's kernels; r06
found a kernel compiled with the packed-FP32 VALU ops returning wrong sums while k_fc_x9t's
bf16-MFMA waves ran beside it, and the two hipBLASLt GEMMs this kernel can replace are outside
the library's build flags.  This repeats rth_fc_bwd at the loop's shape on fixed inputs on one
stream while the learner-shaped x9 FC1 runs on another, and asserts every repetition equal to
the first, and the first equal to fp64 within the FC bound.  A wrong-result check of a
deterministic kernel: one pass, no retry."""
import numpy as np
import pytest
import torch

from reth_amd._lib import call, lib, ptr

pytestmark = pytest.mark.gpu


def test_fc_bwd_exact_beside_concurrent_x9():
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    B, N, K, reps = 512, 512, 3136, 100
    gy = torch.rand((B, N), device=dev, generator=g) * 2 - 1
    gy = gy * (torch.rand((B, N), device=dev, generator=g) < 0.5)
    x = torch.rand((B, K), device=dev, generator=g) * 3 / np.sqrt(B)
    w = (torch.rand((N, K), device=dev, generator=g) * 2 - 1) / np.sqrt(N)
    gx, gw = torch.empty((B, K), device=dev), torch.empty((N, K), device=dev)
    ws = torch.empty(max(lib().rth_fc_bwd_workspace(B, N, K), 16) // 4, device=dev)
    hx, hw = torch.zeros((reps, B, K), device=dev), torch.zeros((reps, N, K), device=dev)
    M = 1024  # the learner's FC1 forward on the other stream
    xl = torch.rand((M, K), device=dev, generator=g)
    b1 = (torch.rand(N, device=dev, generator=g) - 0.5) * 0.1
    yl = torch.empty((M, N), device=dev)
    wsl = torch.empty(max(lib().rth_fc_x9_workspace(M, N, K), 16) // 4, device=dev)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for i in range(reps):
        with torch.cuda.stream(sa):
            gx.fill_(float("nan"))
            gw.fill_(float("nan"))
            call("rth_fc_bwd", ptr(gy), N, ptr(x), K, ptr(w), B, N, K, ptr(gx), ptr(gw), ptr(ws), sa.cuda_stream)
            hx[i].copy_(gx)
            hw[i].copy_(gw)
        with torch.cuda.stream(sb):
            for _ in range(2):
                call("rth_fc_x9", ptr(xl), K, M, ptr(w), N, K, ptr(b1), 1, ptr(yl), ptr(wsl), sb.cuda_stream)
    torch.cuda.synchronize()
    bad = [i for i in range(reps) if not (torch.equal(hx[i], hx[0]) and torch.equal(hw[i], hw[0]))]
    assert not bad, f"{len(bad)} of {reps} repetitions differ (first {bad[:8]})"
    for name, ours, a, b in (("gx", hx[0], gy, w), ("gw", hw[0], gy.t().contiguous(), x)):
        a, b = a.cpu(), b.cpu()
        want = a.double() @ b.double()
        err = (ours.double().cpu() - want).abs().max().item()
        err32 = ((a @ b).double() - want).abs().max().item()
        assert err <= max(4 * err32, 2e-6), (name, err, err32)
